"""ctypes mirror of include/ecdna_ssa.h (the engine's C ABI).

Structs, enums and a `RunSpec` builder that turns the reference's run options
(`SimulationOptions`, src/main.rs:27-44, built by `Cli::build`,
src/clap_app.rs:137-229) into an `ecdna_ssa_params_t` whose host arrays stay
alive as long as the RunSpec does.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

ABI_VERSION = 13
# the oldest library an A/B may load under ECDNA_SSA_ABI_ANY=1: the same Params layout as this ABI (v13 appended
# subsample_cells and reserved1, which an older library would not read)
ABI_SAME_LAYOUT_SINCE = 13

# ecdna_process_t (ProcessType, src/clap_app.rs:311-315)
PURE_BIRTH = 0
BIRTH_DEATH = 1

# ecdna_seg_t (SegregationOptions, src/clap_app.rs:232-238)
SEG_DETERMINISTIC = 0
SEG_BINOMIAL = 1
SEG_BINOMIAL_NO_UNEVEN = 2
SEG_BINOMIAL_NO_NMINUS = 3
SEGREGATION_NAMES = {
    "deterministic": SEG_DETERMINISTIC,
    "binomial": SEG_BINOMIAL,
    "binomial-no-uneven": SEG_BINOMIAL_NO_UNEVEN,
    "binomial-no-nminus": SEG_BINOMIAL_NO_NMINUS,
}

# ecdna_event_t (channel order, src/main.rs:140-145)
EV_PROLIF_NMINUS, EV_PROLIF_NPLUS, EV_DEATH_NMINUS, EV_DEATH_NPLUS = 0, 1, 2, 3

# ecdna_stop_t
STOP_NONE, STOP_MAX_CELLS, STOP_MAX_TIME, STOP_MAX_ITER, STOP_ABSORBING, STOP_ERROR = range(6)
STOP_NAMES = ["None", "MaxCells", "MaxTime", "MaxIter", "Absorbing", "Error"]

# ecdna_rep_error_t
REP_OK, REP_ERR_OVERFLOW, REP_ERR_EMPTY, REP_ERR_CELL_CAP, REP_ERR_REJECTION, REP_ERR_INTERNAL = range(6)

FLAG_TIME_F32 = 0x1
FLAG_BD_CAP_COMPAT = 0x2
FLAG_EVENT_HASH = 0x4
FLAG_SNAPSHOT_ROWS = 0x8

OK = 0
E_INVALID, E_HIP, E_NOMEM, E_NODEVICE, E_STATE, E_COMM = -1, -2, -3, -4, -5, -6
COMM_ID_BYTES = 128

MAX_ITER = 1_000_000_000  # src/main.rs:23
MAX_CELLS = 1_000_000_000  # src/main.rs:25


class Rates(C.Structure):
    _fields_ = [("b0", C.c_float), ("b1", C.c_float), ("d0", C.c_float), ("d1", C.c_float)]


class Params(C.Structure):
    _fields_ = [
        ("process", C.c_int32),
        ("segregation", C.c_int32),
        ("rates", C.POINTER(Rates)),
        ("n_param_sets", C.c_uint32),
        ("hist_bins", C.c_uint32),
        ("reps_per_set", C.c_uint64),
        ("seed", C.c_uint64),
        ("first_replicate", C.c_uint64),
        ("n_replicates", C.c_uint64),
        ("max_cells", C.c_uint64),
        ("max_time", C.c_double),
        ("max_iter", C.c_uint64),
        ("cell_cap", C.c_uint32),
        ("flags", C.c_uint32),
        ("init_copies", C.POINTER(C.c_uint16)),
        ("init_nplus", C.c_uint32),
        ("bin_kmax", C.c_uint32),
        ("init_nminus", C.c_uint64),
        ("init_set_offsets", C.POINTER(C.c_uint32)),
        ("init_set_nminus", C.POINTER(C.c_uint64)),
        ("device", C.c_int32),
        ("big_cap", C.c_uint32),
        ("snapshot_cells", C.POINTER(C.c_uint64)),
        ("n_snapshots", C.c_uint32),
        ("replicate_stride", C.c_uint32),
        ("stats_target_hist", C.POINTER(C.c_uint64)),
        ("set_cost_hint", C.POINTER(C.c_float)),
        ("max_workgroups", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("subsample_cells", C.c_uint32),
        ("reserved1", C.c_uint32),
    ]


class Ext(C.Structure):
    """ecdna_ssa_ext_t: the extension block of ecdna_ssa_ctx_create_ext (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("snapshot_stats", C.c_uint32),
        ("snapshot_target_hists", C.POINTER(C.c_uint64)),
        ("snapshot_subsample_cells", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Passages(C.Structure):
    """ecdna_ssa_passages_t: the passage block of ecdna_ssa_ctx_create_passages (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_passages", C.c_uint32),
        ("passage_cells", C.c_uint32),
        ("reserved", C.c_uint32),
        ("passage_target_hists", C.POINTER(C.c_uint64)),
    ]


# ecdna_accept_source_t: the statistics ecdna_ssa_ctx_accept tests (added within ABI v13)
ACCEPT_FINAL, ACCEPT_SAMPLE, ACCEPT_SNAPSHOTS, ACCEPT_SNAPSHOT_SAMPLES, ACCEPT_PASSAGES, ACCEPT_PASSAGE_SAMPLES = range(6)
# (6 and 7 are not sources.) The cohort's records, T = n_targets: timepoint p is target p (ecdna_ssa_cohort_t)
ACCEPT_COHORT, ACCEPT_COHORT_SAMPLES = 8, 9
# (10 and 11 are not sources.) The records of the last ecdna_ssa_ctx_rescore, T = its P (ecdna_ssa_keep_t)
ACCEPT_RESCORED = 12
# The records of the last ecdna_ssa_ctx_rescore_timepoints, T = the context's snapshots or growth phases
# (ecdna_ssa_keep_timepoints_t)
ACCEPT_RESCORED_TIMEPOINTS = 13
ACCEPT_MAX_THRESHOLDS = 32
COHORT_MAX_TARGETS = 64
KEPT_GUARD = 0xFFFFFFFF  # both words of the header of a kept sample the guard ended (keep mapping v1)


class Keep(C.Structure):
    """ecdna_ssa_keep_t: the keep block of ecdna_ssa_ctx_create_keep (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("keep_cells", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class KeepTimepoints(C.Structure):
    """ecdna_ssa_keep_timepoints_t: the timepoint keep block of ecdna_ssa_ctx_create_keep_timepoints (added within ABI
    v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("keep_cells", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class Rescore(C.Structure):
    """ecdna_ssa_rescore_t: the block of ecdna_ssa_ctx_rescore_sized — the kept samples scored against each target on
    its own number of measured cells (added within ABI v13; thinning mapping v1)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_targets", C.c_uint32),
        ("target_hists", C.POINTER(C.c_uint64)),
        ("sample_cells", C.POINTER(C.c_uint32)),
        ("sample_draws", C.POINTER(C.c_uint32)),
        ("reserved", C.c_uint64),
    ]


THIN_MAX_DRAW = 63  # the draw index of a thinning takes 6 bits (thinning mapping v1)


class Kept(C.Structure):
    """ecdna_kept_t: one kept sample's header, its N- and N+ cell counts."""

    _fields_ = [("nminus", C.c_uint32), ("nplus", C.c_uint32)]


KEPT_DTYPE = np.dtype([("nminus", "<u4"), ("nplus", "<u4")])
assert KEPT_DTYPE.itemsize == C.sizeof(Kept) == 8


class Cohort(C.Structure):
    """ecdna_ssa_cohort_t: the cohort block of ecdna_ssa_ctx_create_cohort (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_targets", C.c_uint32),
        ("target_hists", C.POINTER(C.c_uint64)),
        ("sample_cells", C.POINTER(C.c_uint32)),
        ("reserved", C.c_uint64),
    ]


class AcceptThreshold(C.Structure):
    """ecdna_accept_threshold_t: one threshold row, the largest accepted value of each distance (inf: off)."""

    _fields_ = [("ks", C.c_double), ("mean_rel", C.c_double), ("entropy_rel", C.c_double),
                ("frequency_diff", C.c_double)]


class Accept(C.Structure):
    """ecdna_ssa_accept_t: the argument block of ecdna_ssa_ctx_accept (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("source", C.c_uint32),
        ("n_thresholds", C.c_uint32),
        ("list_threshold", C.c_uint32),
        ("thresholds", C.POINTER(AcceptThreshold)),
        ("timepoint_mask", C.c_uint64),
        ("list_capacity", C.c_uint64),
        ("reserved", C.c_uint64),
    ]


SELECT_MAX_RANKS = 32
SELECT_PASSES = 8  # 8 bits of the 64-bit key per pass
SELECT_FIELDS = ("ks", "mean_rel", "entropy_rel", "frequency_diff")  # the distance order of the select's arrays


class AcceptDraws(C.Structure):
    """ecdna_ssa_accept_draws_t: the block of ecdna_ssa_ctx_accept_draws — acceptance counted over a range of thinning
    draws of the kept samples (added within ABI v13; thinned acceptance mapping v1)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("timepoints", C.c_uint32),
        ("n_targets", C.c_uint32),
        ("target_hists", C.POINTER(C.c_uint64)),
        ("sample_cells", C.POINTER(C.c_uint32)),
        ("first_draw", C.c_uint32),
        ("n_draws", C.c_uint32),
        ("n_thresholds", C.c_uint32),
        ("thresholds", C.POINTER(AcceptThreshold)),
        ("timepoint_mask", C.c_uint64),
        ("reserved", C.c_uint64),
    ]


ACCEPT_DRAWS_MAX = 64  # thinning draws of one kept sample: the draw index takes 6 bits


class Select(C.Structure):
    """ecdna_ssa_select_t: the argument block of ecdna_ssa_ctx_select (added within ABI v13)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("source", C.c_uint32),
        ("timepoint_mask", C.c_uint64),
        ("n_ranks", C.c_uint32),
        ("reserved", C.c_uint32),
        ("ranks", C.POINTER(C.c_uint64)),
        ("fractions", C.POINTER(C.c_double)),
    ]


_MASK64 = (1 << 64) - 1


def passage_seed(seed: int, g: int) -> int:
    """The Philox key seed_g of growth phase g (passage mapping v1, include/ecdna_ssa.h): the seed for phase 0, else
    the splitmix64 finaliser of seed + g * 0x9E3779B97F4A7C15 (mod 2^64)."""
    if g == 0:
        return int(seed) & _MASK64
    z = (int(seed) + g * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


STATS_DTYPE = np.dtype([("mean", "<f8"), ("entropy", "<f8"), ("frequency", "<f8"), ("ks", "<f8"),
                        ("mean_rel", "<f8"), ("entropy_rel", "<f8"), ("frequency_diff", "<f8"), ("cells", "<u8")])
assert STATS_DTYPE.itemsize == 64
FLAG_REP_STATS = 0x10
FLAG_BIN_STORE = 0x20  # cells binned by copy number; bin_kmax = 64 or 256
# the reference's own draw structure (ChaCha8 streams seed*10+r, first reaction, rand_distr samplers, f32 time;
# row store only): seed for seed the oracle's compat mode
FLAG_REFERENCE_DRAWS = 0x40
FLAG_ALL = 0x7F  # every defined flag (ecdna_ssa_ctx_create rejects other bits since ABI v11)


# ecdna_ssa_instance_t (ABI v7): the kernel instance a context launches (ecdna_ssa_ctx_instance)
KERNEL_KINDS = {0: "ssa_stepper (rows)", 1: "ssa_stepper_bins (bins)", 2: "ssa_stepper_refdraws (reference draws)"}
SCHEDULE_NAMES = {-1: "n/a", 0: "occupancy-first", 1: "max-ILP", 2: "occupancy-first, 128-VGPR cap", 3: "max-ILP, paired lanes"}


class Instance(C.Structure):
    _fields_ = [
        ("kernel", C.c_int32),
        ("schedule", C.c_int32),
        ("paired", C.c_int32),
        ("rotation", C.c_int32),
        ("rot_tick_log2", C.c_int32),
        ("drain_control", C.c_int32),
        ("cost_order", C.c_int32),
        ("runtime_flags", C.c_int32),
        ("bin_kmax", C.c_uint32),
        ("bin_c32", C.c_uint32),
        ("block_lanes", C.c_uint32),
        ("blocks_per_cu", C.c_uint32),
        ("cus", C.c_uint32),
        ("n_chunks", C.c_uint32),
        ("vgprs", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("scratch_bytes", C.c_uint32),
        ("window", C.c_uint32),
        ("chunk_replicates", C.c_uint64),
        ("grid_lanes", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f, _ in self._fields_}
        d["kernel_name"] = KERNEL_KINDS.get(d["kernel"], "?")
        d["schedule_name"] = SCHEDULE_NAMES.get(d["schedule"], "?")
        return d


def _signatures():
    """Every function include/ecdna_ssa.h declares, in its order of introduction: (name, restype, argtypes, added).
    `added`: None for the calls every library of this ABI version has; for those added within v13, what they brought —
    a same-box A/B may load a v13 library built before them, which runs everything else (engine._lib_with)."""
    P, V, I, U32, U64 = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    create = [P(Params), P(Ext), P(Passages), P(Cohort), P(Keep), P(KeepTimepoints)]  # the create chain's blocks
    base = [
        ("abi_version", I, []), ("strerror", C.c_char_p, [I]), ("last_error_message", C.c_char_p, []),
        ("device_count", I, []), ("run", I, [P(Params), V, V, V, V]), ("ctx_create", I, create[:1] + [P(V)]),
        ("ctx_set_outputs", I, [V, V, V]), ("ctx_launch", I, [V, V]), ("ctx_sync", I, [V, P(C.c_float), P(C.c_float)]),
        ("ctx_device_outputs", I, [V, P(V), P(V)]), ("ctx_download", I, [V, V, V, V, V]),
        ("ctx_download_snapshots", I, [V, V, V]), ("ctx_download_stats", I, [V, V]),
        ("ctx_download_sample", I, [V, V, V]), ("ctx_download_rng_words", I, [V, V]),
        ("ctx_row_stride", C.c_int64, [V]), ("ctx_geometry", I, [V, P(U64), P(U64)]),
        ("ctx_instance", I, [V, P(Instance)]), ("ctx_destroy", I, [V]), ("comm_unique_id", I, [V]),
        ("comm_init_rank", I, [V, I, I, I, P(V)]), ("comm_init_all", I, [I, P(I), P(V)]), ("comm_destroy", I, [V]),
        ("reduce_hist", I, [V, V, V, U32, U32, V]), ("ctx_reduce", I, [V, V]),
    ]
    within_v13 = {
        "per-snapshot statistics": [("ctx_create_ext", create[:2] + [P(V)]), ("ctx_download_snapshot_stats", [V] * 5)],
        "serial passaging": [("ctx_create_passages", create[:3] + [P(V)]), ("ctx_download_passages", [V] * 7)],
        "ABC rejection on the GPU": [("ctx_accept", [V, P(Accept)]),
                                     ("ctx_download_accept", [V, V, V, P(U64), V, V])],
        "ABC thresholds on the GPU": [("ctx_select", [V, P(Select), P(U64), V, V, V]),
                                      ("ctx_select_digits", [V, U32, U64, U32, U32, V, V])],
        "a cohort of targets": [("ctx_create_cohort", create[:4] + [P(V)]), ("ctx_download_cohort", [V, V, V])],
        "kept samples": [("ctx_create_keep", create[:5] + [P(V)]), ("ctx_rescore", [V, U32, V]),
                         ("ctx_download_rescored", [V, V]), ("ctx_pool_accepted", [V, U32, V]),
                         ("ctx_download_kept", [V, U64, V, V, V])],
        "kept timepoint samples": [("ctx_create_keep_timepoints", create + [P(V)]), ("ctx_rescore_timepoints", [V, V]),
                                   ("ctx_download_rescored_timepoints", [V, V]),
                                   ("ctx_pool_accepted_timepoints", [V, U32, V]),
                                   ("ctx_download_kept_timepoints", [V, U64, V, V, V])],
        "sized rescoring": [("ctx_rescore_sized", [V, P(Rescore)]), ("ctx_rescore_timepoints_sized", [V, V, V, U32])],
        "acceptance over repeated thinnings": [("ctx_accept_draws", [V, P(AcceptDraws)]),
                                               ("ctx_download_accept_draws", [V, V, V])],
        # (c, block, threshold, out_thinned [n_targets][n_param_sets][hist_bins], out_kept [n_slices][..][..])
        "pooling over thinning draws": [("ctx_pool_draws", [V, P(AcceptDraws), U32, V, V])],
        # (c, block without threshold rows, n_ranks, ranks, fractions, out_population, out_ranks, out_values,
        # out_counts_le) and (c, block, pass, n_prefixes, prefixes, out_hist)
        "ABC thresholds over thinning draws": [("ctx_select_draws", [V, P(AcceptDraws), U32, V, V, P(U64), V, V, V]),
                                               ("ctx_select_draws_digits", [V, P(AcceptDraws), U32, U32, V, V])],
    }
    rows = [("ecdna_ssa_" + n, r, a, None) for n, r, a in base]
    return rows + [("ecdna_ssa_" + n, I, a, what) for what, calls in within_v13.items() for n, a in calls]


SIGNATURES = _signatures()
_ARGTYPES = {name: argtypes for name, _, argtypes, _ in SIGNATURES}
POOL_DRAWS_ARGTYPES = _ARGTYPES["ecdna_ssa_ctx_pool_draws"]
SELECT_DRAWS_ARGTYPES = _ARGTYPES["ecdna_ssa_ctx_select_draws"]
SELECT_DRAWS_DIGITS_ARGTYPES = _ARGTYPES["ecdna_ssa_ctx_select_draws_digits"]


SNAPSHOT_DTYPE = np.dtype([("time", "<f8"), ("nminus", "<u8"), ("nplus", "<u8"), ("taken", "<u4"),
                           ("reserved", "<u4")])
assert SNAPSHOT_DTYPE.itemsize == 32


def default_snapshots(cells: int, n_snapshots: int = 11):
    """build_snapshots_from_cells (src/clap_app.rs:121-134): [1, 1+dx, ..., cells], dx = cells / 10."""
    dx = cells // (n_snapshots - 1)
    x = [1] * n_snapshots
    for i in range(1, n_snapshots - 1):
        x[i] = x[i - 1] + dx
    x[n_snapshots - 1] = cells
    return sorted(x)


SUMMARY_DTYPE = np.dtype(
    [
        ("nminus", "<u8"),
        ("nplus", "<u8"),
        ("iters", "<u8"),
        ("events_by_type", "<u8", (4,)),
        ("uneven", "<u8"),
        ("time", "<f8"),
        ("event_hash", "<u8"),
        ("stop_reason", "<u4"),
        ("error", "<u4"),
    ]
)
assert SUMMARY_DTYPE.itemsize == 88

TOTALS_DTYPE = np.dtype(
    [
        ("replicates", "<u8"),
        ("events", "<u8"),
        ("events_by_type", "<u8", (4,)),
        ("uneven", "<u8"),
        ("nminus", "<u8"),
        ("nplus", "<u8"),
        ("stop_reasons", "<u8", (6,)),
        ("errors", "<u8"),
    ]
)
assert TOTALS_DTYPE.itemsize == 128


def _ptr(arr: Optional[np.ndarray], ctype):
    if arr is None:
        return C.POINTER(ctype)()
    return arr.ctypes.data_as(C.POINTER(ctype))


@dataclass
class RunSpec:
    """One run of `n_replicates` replicates — the batched form of run_simulations (src/main.rs:55-211)."""

    process: int = PURE_BIRTH
    segregation: int = SEG_BINOMIAL
    rates: Sequence[Sequence[float]] = ((1.0, 1.0, 0.0, 0.0),)  # [b0, b1, d0, d1] per set
    reps_per_set: Optional[int] = None  # default: all replicates in set 0
    seed: int = 26  # src/clap_app.rs:63
    first_replicate: int = 0
    n_replicates: int = 12  # src/clap_app.rs:89
    replicate_stride: int = 1  # replicate i has global id first_replicate + i * replicate_stride
    max_cells: int = 1000  # src/clap_app.rs:149
    max_time: Optional[float] = None  # default: floor(log2(cells) + 4), src/clap_app.rs:151
    max_iter: int = MAX_ITER
    cell_cap: Optional[int] = None  # default: max(max_cells, largest initial N+ count)
    hist_bins: int = 1025
    flags: int = FLAG_EVENT_HASH
    init: Optional[Dict[int, int]] = None  # histogram {copies: cells}; default {1: 1} (src/clap_app.rs:188-191)
    init_per_set: Optional[List[Dict[int, int]]] = None
    device: int = 0
    snapshots: Optional[Sequence[int]] = None  # cell counts (sorted here); None = no snapshots
    stats_target: Optional[Sequence[int]] = None  # target histogram [hist_bins] for ABC distances
    bin_kmax: int = 0  # FLAG_BIN_STORE: binned copy numbers 1..bin_kmax (0 = 64)
    set_cost_hint: Optional[Sequence[float]] = None  # per set: start costlier sets first (speed only)
    big_cap: int = 0  # FLAG_BIN_STORE: large-k row capacity (cells with k > bin_kmax); 0 = cell_cap
    max_workgroups: int = 0  # persistent-grid cap (0 = fill the device); for contexts sharing a GPU (speed only)
    # end-of-run subsampling on the GPU (ABI v13): statistics and histogram of a sample of this many cells of every
    # replicate's final population (Result.sample_stats / sample_hist); 0 = off; needs FLAG_REP_STATS; <= 4096
    subsample_cells: int = 0
    # per-snapshot ABC statistics on the GPU (ecdna_ssa_ext_t, within ABI v13): the statistics of every replicate's
    # state at every snapshot (Result.snapshot_stats / snapshot_hist), distances against snapshot_targets[s]
    # ([S][hist_bins], or None: no distances), and of a sample of snapshot_subsample_cells of its cells
    # (Result.snapshot_sample_stats / snapshot_sample_hist; 0 = off, <= 4096). Needs snapshots and FLAG_REP_STATS;
    # without FLAG_SNAPSHOT_ROWS the snapshot rows stay on the device, one chunk at a time
    snapshot_stats: bool = False
    snapshot_targets: Optional[Sequence[Sequence[int]]] = None
    snapshot_subsample_cells: int = 0
    # serial passaging on the GPU (ecdna_ssa_passages_t, within ABI v13; the reference's cell-line strategy): n_passages
    # growth phases per replicate, each after the first regrown from a sample of passage_cells cells of the previous
    # one (Result.passages; distances against passage_targets[g], [G][hist_bins], or None: stats_target for all).
    # 0 = an ordinary run. Needs FLAG_REP_STATS; no snapshots, no subsample_cells, no reference draws
    n_passages: int = 0
    passage_cells: int = 0
    passage_targets: Optional[Sequence[Sequence[int]]] = None
    # a cohort of targets scored against this one run on the GPU (ecdna_ssa_cohort_t, within ABI v13; cohort mapping
    # v1): cohort_targets [P][hist_bins], P <= 64 — several patients, or biopsies, each with its own histogram — and
    # cohort_sample_cells [P], target p's number of measured cells (None: no samples). Result.cohort holds every
    # replicate's records against every target. Needs FLAG_REP_STATS; no passages, no snapshot_stats
    cohort_targets: Optional[Sequence[Sequence[int]]] = None
    cohort_sample_cells: Optional[Sequence[int]] = None
    # every replicate's sample of keep_cells cells kept on the GPU (ecdna_ssa_keep_t, within ABI v13; keep mapping v1),
    # for Context.rescore, .pool_accepted and .download_kept after the sweep. None = no block. Needs FLAG_REP_STATS;
    # 1 .. 4096; no passages. n_replicates * keep_cells * 2 bytes of device memory
    keep_cells: Optional[int] = None
    # the sample of keep_timepoint_cells cells of every timepoint kept on the GPU (ecdna_ssa_keep_timepoints_t, within
    # ABI v13; timepoint keep mapping v1): every snapshot of a run with snapshot_stats, or every growth phase of a
    # passage run (then it must equal passage_cells), for Context.rescore_timepoints, .pool_accepted_timepoints and
    # .download_kept_timepoints after the sweep. None = no block. Needs FLAG_REP_STATS; 1 .. 4096.
    # T * n_replicates * (2 * keep_timepoint_cells + 8) bytes of device memory
    keep_timepoint_cells: Optional[int] = None
    _keep: list = field(default_factory=list, repr=False)
    _keep_cohort: list = field(default_factory=list, repr=False)
    _keep_ext: list = field(default_factory=list, repr=False)
    _keep_pas: list = field(default_factory=list, repr=False)

    def stride(self) -> int:
        """The id step as the C ABI reads it: replicate_stride 0 means 1 (include/ecdna_ssa.h)."""
        return self.replicate_stride if self.replicate_stride else 1

    def replicate_ids(self) -> np.ndarray:
        """Global ids of the call's replicates, in summary order."""
        return self.first_replicate + np.arange(self.n_replicates, dtype=np.uint64) * np.uint64(self.stride())

    def last_replicate(self) -> int:
        return self.first_replicate + max(0, self.n_replicates - 1) * self.stride()

    def resolved_max_time(self) -> float:
        if self.max_time is not None:
            return float(self.max_time)
        # (f32::log2(cells as f32) + 4f32) as u64, then `years as f32`
        years = np.log2(np.float32(self.max_cells)) + np.float32(4.0)
        return float(np.float32(int(years)))

    @staticmethod
    def _copies_of(hist: Dict[int, int]):
        """EcDNADistribution::new from a histogram: n- = hist[0], one u16 per N+ cell, keys sorted
        (the reference iterates a HashMap, whose order is random per process: SURVEY.md App. A.2)."""
        nminus = int(hist.get(0, 0))
        cells = []
        for k in sorted(int(k) for k in hist if int(k) > 0):
            if k > 65535:
                raise ValueError(f"copy number {k} does not fit u16")
            cells.extend([k] * int(hist[k]))
        return np.asarray(cells, dtype=np.uint16), nminus

    def params(self) -> Params:
        # ctypes silently masks values that do not fit a field (a stride of 2^32 would become 0, i.e. 1):
        # reject them here instead
        for name, bits in (("replicate_stride", 32), ("big_cap", 32), ("bin_kmax", 32), ("hist_bins", 32),
                           ("subsample_cells", 32),
                           ("n_replicates", 64), ("first_replicate", 64), ("seed", 64), ("max_cells", 64),
                           ("max_iter", 64)):
            v = getattr(self, name)
            if not (0 <= int(v) < (1 << bits)):
                raise ValueError(f"{name} = {v} does not fit the ABI's u{bits} field")
        if self.cell_cap is not None and not (0 <= int(self.cell_cap) < (1 << 32)):
            raise ValueError(f"cell_cap = {self.cell_cap} does not fit the ABI's u32 field")
        self._keep = []
        rates = np.asarray(self.rates, dtype=np.float32).reshape(-1, 4)
        n_sets = rates.shape[0]
        rates_arr = (Rates * n_sets)(*[Rates(*map(float, r)) for r in rates])
        self._keep.append(rates_arr)
        p = Params()
        p.process = self.process
        p.segregation = self.segregation
        p.rates = C.cast(rates_arr, C.POINTER(Rates))
        p.n_param_sets = n_sets
        p.hist_bins = self.hist_bins
        rps = self.reps_per_set
        if rps is None:
            rps = max(1, self.last_replicate() + 1)
        p.reps_per_set = rps
        p.seed = self.seed
        p.first_replicate = self.first_replicate
        p.n_replicates = self.n_replicates
        p.replicate_stride = self.replicate_stride
        p.max_cells = self.max_cells
        p.max_time = self.resolved_max_time()
        p.max_iter = self.max_iter
        p.flags = self.flags
        p.bin_kmax = self.bin_kmax
        p.big_cap = self.big_cap
        p.max_workgroups = self.max_workgroups
        p.subsample_cells = self.subsample_cells
        p.device = self.device
        if self.snapshots:
            snaps = np.asarray(sorted(int(x) for x in self.snapshots), dtype=np.uint64)
            self._keep.append(snaps)
            p.snapshot_cells = _ptr(snaps, C.c_uint64)
            p.n_snapshots = len(snaps)
        if self.set_cost_hint is not None:
            hint = np.asarray(self.set_cost_hint, dtype=np.float32)
            if hint.shape != (n_sets,):
                raise ValueError("set_cost_hint needs one value per parameter set")
            self._keep.append(hint)
            p.set_cost_hint = _ptr(hint, C.c_float)
        if self.stats_target is not None:
            tgt = np.asarray(self.stats_target, dtype=np.uint64)
            if tgt.shape != (self.hist_bins,):
                raise ValueError("stats_target must have hist_bins entries")
            self._keep.append(tgt)
            p.stats_target_hist = _ptr(tgt, C.c_uint64)
        max_np = 0
        if self.init_per_set is not None:
            if len(self.init_per_set) != n_sets:
                raise ValueError("init_per_set needs one histogram per parameter set")
            parts = [self._copies_of(h) for h in self.init_per_set]
            offs = np.zeros(n_sets + 1, dtype=np.uint32)
            offs[1:] = np.cumsum([len(c) for c, _ in parts])
            copies = np.concatenate([c for c, _ in parts]).astype(np.uint16) if offs[-1] else np.zeros(1, np.uint16)
            nms = np.asarray([nm for _, nm in parts], dtype=np.uint64)
            self._keep += [copies, offs, nms]
            p.init_copies = _ptr(copies, C.c_uint16)
            p.init_nplus = 0
            p.init_nminus = 0
            p.init_set_offsets = _ptr(offs, C.c_uint32)
            p.init_set_nminus = _ptr(nms, C.c_uint64)
            max_np = int(np.max(np.diff(offs))) if n_sets else 0
        else:
            copies, nm = self._copies_of(self.init if self.init is not None else {1: 1})
            buf = copies if len(copies) else np.zeros(1, np.uint16)
            self._keep.append(buf)
            p.init_copies = _ptr(buf, C.c_uint16)
            p.init_nplus = len(copies)
            p.init_nminus = nm
            max_np = len(copies)
            parts = [(copies, nm)]
        # populations are u32 (include/ecdna_ssa.h): the library refuses an initial n- + n+ of 2^32 or more, and so does
        # the spec, before the engine or the oracle sees it
        for c, nm in parts:
            if nm + len(c) >= 1 << 32:
                raise ValueError(f"initial cells (N- {nm} plus N+ {len(c)}) must be < 2^32")
        cap = self.cell_cap
        if cap is None:
            cap = max(int(min(self.max_cells, 2**32 - 1)), max_np, 1)
        p.cell_cap = cap
        return p

    def ext(self) -> Optional[Ext]:
        """The extension block this spec asks for, or None: the context is then made by ecdna_ssa_ctx_create."""
        if not (self.snapshot_stats or self.snapshot_targets is not None or self.snapshot_subsample_cells):
            return None
        if not (0 <= int(self.snapshot_subsample_cells) < (1 << 32)):
            raise ValueError(f"snapshot_subsample_cells = {self.snapshot_subsample_cells} does not fit the ABI's u32 field")
        self._keep_ext = []
        e = Ext()
        e.struct_size = C.sizeof(Ext)
        e.snapshot_stats = 1 if self.snapshot_stats else 0
        e.snapshot_subsample_cells = self.snapshot_subsample_cells
        if self.snapshot_targets is not None:
            tgt = np.ascontiguousarray(self.snapshot_targets, dtype=np.uint64)
            if tgt.shape != (len(self.snapshots or ()), self.hist_bins):
                raise ValueError("snapshot_targets must have one histogram of hist_bins entries per snapshot")
            self._keep_ext.append(tgt)
            e.snapshot_target_hists = _ptr(tgt, C.c_uint64)
        return e

    def passages(self) -> Optional[Passages]:
        """The passage block this spec asks for, or None: the context is then made without ecdna_ssa_ctx_create_passages."""
        if not (self.n_passages or self.passage_cells or self.passage_targets is not None):
            return None
        for name in ("n_passages", "passage_cells"):
            if not (0 <= int(getattr(self, name)) < (1 << 32)):
                raise ValueError(f"{name} = {getattr(self, name)} does not fit the ABI's u32 field")
        self._keep_pas = []
        b = Passages()
        b.struct_size = C.sizeof(Passages)
        b.n_passages = self.n_passages
        b.passage_cells = self.passage_cells
        if self.passage_targets is not None:
            tgt = np.ascontiguousarray(self.passage_targets, dtype=np.uint64)
            if tgt.shape != (self.n_passages, self.hist_bins):
                raise ValueError("passage_targets must have one histogram of hist_bins entries per passage")
            self._keep_pas.append(tgt)
            b.passage_target_hists = _ptr(tgt, C.c_uint64)
        return b

    def cohort(self) -> Optional[Cohort]:
        """The cohort block this spec asks for, or None (no cohort_targets): the context is then made without
        ecdna_ssa_ctx_create_cohort."""
        if self.cohort_targets is None:
            if self.cohort_sample_cells is not None:
                raise ValueError("cohort_sample_cells needs cohort_targets")
            return None
        self._keep_cohort = []
        tgt = np.ascontiguousarray(self.cohort_targets, dtype=np.uint64)
        if tgt.ndim != 2 or tgt.shape[1] != self.hist_bins:
            raise ValueError("cohort_targets must be [P][hist_bins]: one histogram of hist_bins entries per target")
        b = Cohort()
        b.struct_size = C.sizeof(Cohort)
        b.n_targets = tgt.shape[0]
        self._keep_cohort.append(tgt)
        b.target_hists = _ptr(tgt, C.c_uint64)
        if self.cohort_sample_cells is not None:
            for m in self.cohort_sample_cells:
                if not (0 <= int(m) < (1 << 32)):
                    raise ValueError(f"cohort_sample_cells entry {m} does not fit the ABI's u32 field")
            cells = np.asarray([int(m) for m in self.cohort_sample_cells], dtype=np.uint32)
            if cells.shape != (tgt.shape[0],):
                raise ValueError("cohort_sample_cells needs one sample size per target")
            self._keep_cohort.append(cells)
            b.sample_cells = _ptr(cells, C.c_uint32)
        return b

    def keep(self) -> Optional[Keep]:
        """The keep block this spec asks for, or None (keep_cells is None): the context is then made without
        ecdna_ssa_ctx_create_keep."""
        if self.keep_cells is None:
            return None
        if not (0 <= int(self.keep_cells) < (1 << 32)):
            raise ValueError(f"keep_cells = {self.keep_cells} does not fit the ABI's u32 field")
        b = Keep()
        b.struct_size = C.sizeof(Keep)
        b.keep_cells = int(self.keep_cells)
        return b

    def timepoints(self) -> int:
        """T of the timepoint keep block: the growth phases of a passage run, else the snapshots of a run with
        snapshot_stats, else 0."""
        if self.n_passages:
            return int(self.n_passages)
        return len(self.snapshots or ()) if self.snapshot_stats else 0

    def keep_timepoints(self) -> Optional[KeepTimepoints]:
        """The timepoint keep block this spec asks for, or None (keep_timepoint_cells is None): the context is then
        made without ecdna_ssa_ctx_create_keep_timepoints."""
        if self.keep_timepoint_cells is None:
            return None
        if not (0 <= int(self.keep_timepoint_cells) < (1 << 32)):
            raise ValueError(f"keep_timepoint_cells = {self.keep_timepoint_cells} does not fit the ABI's u32 field")
        b = KeepTimepoints()
        b.struct_size = C.sizeof(KeepTimepoints)
        b.keep_cells = int(self.keep_timepoint_cells)
        return b


def cost_hint(rates: Sequence[Sequence[float]], inits: Optional[Sequence[Dict[int, int]]] = None) -> List[float]:
    """A rough relative cost per replicate of each parameter set, for RunSpec.set_cost_hint: events to grow
    a birth-death population scale with (b1 + d1) / (b1 - d1) (net growth per event of the N+ type), and
    an event costs more as copy numbers grow (2k segregation bits beyond the first Philox words, cells
    beyond the LDS bins): factor 1 + mean initial copy number / 16. Only the ORDER of the values matters
    (longest-processing-time starts); a poor estimate costs speed, never results."""
    out = []
    for s, r in enumerate(rates):
        b1, d1 = float(r[1]), float(r[3])
        events = (b1 + d1) / max(b1 - d1, 0.05)
        k = 1.0
        if inits is not None:
            h = {int(key): int(v) for key, v in inits[s].items() if int(key) > 0}
            if h:
                k = sum(key * v for key, v in h.items()) / max(1, sum(h.values()))
        out.append(events * (1.0 + k / 16.0))
    return out


def summaries_array(n: int) -> np.ndarray:
    return np.zeros(n, dtype=SUMMARY_DTYPE)


def totals_array(n_sets: int) -> np.ndarray:
    return np.zeros(n_sets, dtype=TOTALS_DTYPE)


def as_ptr(arr: np.ndarray):
    return C.c_void_p(arr.ctypes.data)
