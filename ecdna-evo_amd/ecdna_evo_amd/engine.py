"""ctypes bindings of libecdna_ssa.so (include/ecdna_ssa.h) — the product's host-side entry points.

`run()` is the batched replacement of the reference's per-replicate `sosa::simulate` calls
(src/main.rs:92-99, 166-173) mapped by rayon over replicate ids (src/main.rs:212-225); `Context`
keeps inputs and outputs resident in HBM for repeated launches and multi-GPU reductions.

There is no CPU fallback: if the HIP library is missing or no gfx950 device is present, every
entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import abi

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # .../ecdna-evo_amd
# ECDNA_SSA_LIB: development override (same-box A/B of two builds, tools/ab_build.sh)
LIB_PATH = os.environ.get("ECDNA_SSA_LIB") or os.path.join(PKG_ROOT, "lib", "libecdna_ssa.so")

EXPORTS = [name for name, _, _, _ in abi.SIGNATURES]


class EngineError(RuntimeError):
    pass


_lib = None


def _ensure_single_hip_runtime():
    # torch ships its own libamdhip64.so.7; importing it first makes the soname resolve to that copy,
    # so the engine and torch (streams, RCCL) share one HIP runtime in a process that uses both.
    if os.environ.get("ECDNA_NO_TORCH_PRELOAD"):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing: build it with `make -C ecdna-evo_amd` (or __graft_entry__.build())")
    _ensure_single_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, restype, argtypes, added in abi.SIGNATURES:
        # (added within v13: a same-box A/B may load a v13 library built before the call, which runs everything else;
        # _lib_with raises when such a library is asked for it. A call of the version's baseline must be there.)
        if added is None or hasattr(L, name):
            fn = getattr(L, name)
            fn.restype = restype
            fn.argtypes = argtypes
    ver = L.ecdna_ssa_abi_version()
    # (a same-box A/B, tools/ab_build.sh, may load a library of an earlier ABI version whose Params layout is this
    # one's: ECDNA_SSA_ABI_ANY=1 accepts versions ABI_SAME_LAYOUT_SINCE .. ABI_VERSION, never a newer one;
    # results then follow that library's draw mapping)
    any_ok = os.environ.get("ECDNA_SSA_ABI_ANY") == "1" and abi.ABI_SAME_LAYOUT_SINCE <= ver <= abi.ABI_VERSION
    if ver != abi.ABI_VERSION and not any_ok:
        raise EngineError("ABI version mismatch between libecdna_ssa.so and ecdna_evo_amd.abi")
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        L = lib()
        raise EngineError(f"{what}: {L.ecdna_ssa_strerror(rc).decode()} ({rc}): "
                          f"{L.ecdna_ssa_last_error_message().decode()}")


_ADDED = {name: added for name, _, _, added in abi.SIGNATURES}


def _lib_with(symbol: str, what: Optional[str] = None):
    """The library, which must export `symbol`: an entry point added within an ABI version, with `what` it brought
    (default: what abi.SIGNATURES says)."""
    if not hasattr(lib(), symbol):
        raise EngineError(f"{LIB_PATH} predates {symbol} ({what or _ADDED[symbol]})")
    return lib()


def _check_u32(name: str, v):
    if not (0 <= int(v) < (1 << 32)):
        raise ValueError(f"{name} = {v} does not fit the ABI's u32 field")


def device_count() -> int:
    return lib().ecdna_ssa_device_count()


class Comm:
    """An RCCL communicator made by the engine's C ABI (ecdna_ssa_comm_init_all / init_rank): the multi-GPU
    reduction of ecdna_ssa_ctx_reduce."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def init_all(devices) -> list:
        devs = (C.c_int * len(devices))(*devices)
        out = (C.c_void_p * len(devices))()
        _check(lib().ecdna_ssa_comm_init_all(len(devices), devs, out), "ecdna_ssa_comm_init_all")
        return [Comm(C.c_void_p(out[i])) for i in range(len(devices))]

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
        _check(lib().ecdna_ssa_comm_unique_id(buf), "ecdna_ssa_comm_unique_id")
        return bytes(buf)

    @staticmethod
    def init_rank(uid: bytes, n_ranks: int, rank: int, device: int) -> "Comm":
        buf = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        _check(lib().ecdna_ssa_comm_init_rank(buf, n_ranks, rank, device, C.byref(h)), "ecdna_ssa_comm_init_rank")
        return Comm(h)

    def close(self):
        if getattr(self, "h", None):
            lib().ecdna_ssa_comm_destroy(self.h)
            self.h = None


class Result:
    def __init__(self, summaries, hist, totals, rows=None, row_stride=0):
        self.summaries = summaries
        self.hist = hist
        self.totals = totals
        self.rows = rows
        self.row_stride = row_stride
        self.snapshots = None  # [n][S] abi.SNAPSHOT_DTYPE
        self.snapshot_rows = None  # [n][S][stride] u16 under FLAG_SNAPSHOT_ROWS
        self.stats = None  # [n] abi.STATS_DTYPE under FLAG_REP_STATS
        # RunSpec.subsample_cells > 0: the statistics of every replicate's end-of-run sample, [n] abi.STATS_DTYPE, and
        # the per-set sum of the samples' histograms, [n_sets][hist_bins] u64 (else None)
        self.sample_stats = None
        self.sample_hist = None
        # RunSpec.snapshot_stats: the statistics of every replicate's state at every snapshot, [n][S] abi.STATS_DTYPE
        # (a snapshot not taken: an empty population), and per snapshot and set the sum of the states' histograms,
        # [S][n_sets][hist_bins] u64; with snapshot_subsample_cells > 0 the same for the samples (else None)
        self.snapshot_stats = None
        self.snapshot_hist = None
        self.snapshot_sample_stats = None
        self.snapshot_sample_hist = None
        self.rng_words = None  # [n] u64 under FLAG_REFERENCE_DRAWS: ChaCha8 stream position at the end
        # RunSpec.n_passages = G > 0: every growth phase's results (PassageResult), each array with a leading G axis;
        # the fields above are then the last phase's
        self.passages = None
        # RunSpec.cohort_targets (P of them): every replicate's records against every target (CohortResult)
        self.cohort = None

    def row(self, i: int) -> np.ndarray:
        return self.rows[i, : int(self.summaries[i]["nplus"])]

    def snapshot_row(self, i: int, s: int) -> np.ndarray:
        return self.snapshot_rows[i, s, : int(self.snapshots[i, s]["nplus"])]


class PassageResult:
    """Every growth phase of a passage run (ecdna_ssa_ctx_download_passages): summaries [G][n], totals [G][n_sets],
    stats and sample_stats [G][n] abi.STATS_DTYPE (the phase's final population and its sample of passage_cells cells),
    hist and sample_hist [G][n_sets][hist_bins] u64."""

    def __init__(self, summaries, totals, stats, sample_stats, hist, sample_hist):
        self.summaries = summaries
        self.totals = totals
        self.stats = stats
        self.sample_stats = sample_stats
        self.hist = hist
        self.sample_hist = sample_hist


class CohortResult:
    """One run scored against a cohort of P targets (ecdna_ssa_ctx_download_cohort, cohort mapping v1): stats [P][n]
    abi.STATS_DTYPE, replicate i's whole final population against target p, and sample_stats [P][n], its sample of
    cohort_sample_cells[p] cells against target p (None without sample sizes)."""

    def __init__(self, stats, sample_stats):
        self.stats = stats
        self.sample_stats = sample_stats


class AcceptResult:
    """What ecdna_ssa_ctx_accept keeps of a run (acceptance mapping v1, include/ecdna_ssa.h): counts [Q][n_sets] u64,
    the replicates accepted per threshold row and parameter set (shards' arrays sum to the whole run's); mask [n] u32,
    bit q = replicate i accepted under row q; n_accepted, the number accepted under the list's row (the whole count,
    even above the capacity); ids [n_listed] u64 and stats [n_listed][T] abi.STATS_DTYPE, the global ids and the source's
    records of the first n_listed = min(n_accepted, list_capacity) of them, in call order."""

    def __init__(self, counts, mask, n_accepted, ids, stats):
        self.counts = counts
        self.mask = mask
        self.n_accepted = n_accepted
        self.ids = ids
        self.stats = stats


class AcceptDrawsResult:
    """What ecdna_ssa_ctx_accept_draws keeps (thinned acceptance mapping v1, include/ecdna_ssa.h): sums [Q][n_sets] u64,
    per threshold row and global parameter set the sum of passes over the call's replicates (shards' arrays sum to the
    whole run's); passes [n][Q] u8, the number of the n_draws thinnings on which replicate i is accepted under row q.
    passes / n_draws estimates the replicate's acceptance probability under measurement noise."""

    def __init__(self, sums, passes, n_draws):
        self.sums = sums
        self.passes = passes
        self.n_draws = n_draws


class PoolDrawsResult:
    """What ecdna_ssa_ctx_pool_draws returns (thinned pooling mapping v1, include/ecdna_ssa.h), per global parameter set:
    thinned [n_targets][n_sets][hist_bins] u64, the pooled histograms of each slot's thinned samples on the draws its
    replicates pass under the threshold row — the posterior predictive of the measurement; kept
    [n_slices][n_sets][hist_bins] u64, the whole kept samples weighted by the number of passing draws. Shards' arrays
    sum to the whole run's."""

    def __init__(self, thinned, kept):
        self.thinned = thinned
        self.kept = kept


class SelectResult:
    """Order statistics of the four distances among the error-free replicates (select mapping v1, include/ecdna_ssa.h):
    population, their number M; ranks [K] u64, those asked for or those the fractions map to; values [4][K] f64 and
    counts_le [4][K] u64 in the distance order abi.SELECT_FIELDS: the number whose key is the ranks[j]-th smallest, and
    how many of the M are <= it (a rank above M: +inf and M)."""

    def __init__(self, population, ranks, values, counts_le):
        self.population = population
        self.ranks = ranks
        self.values = values
        self.counts_le = counts_le


def timepoint_mask(timepoints) -> int:
    """The ABI's timepoint_mask of an iterable of participating timepoints (None: 0 = all)."""
    mask = 0
    for t in (timepoints if timepoints is not None else ()):
        if not (0 <= int(t) < 64):
            raise ValueError(f"timepoint {t} does not fit the ABI's 64-bit timepoint_mask")
        mask |= 1 << int(t)
    if timepoints is not None and mask == 0:
        raise ValueError("timepoints is empty (None = all)")
    return mask


def select_ranks(ranks=None, fractions=None):
    """The checked arguments of a select, (ranks [K] u64 or None, fractions [K] f64 or None): exactly one of the two,
    K in 1 .. 32, every rank >= 1 and below 2^64, every fraction in (0, 1]. Raises ValueError otherwise."""
    if (ranks is None) == (fractions is None):
        raise ValueError("exactly one of ranks and fractions must be given")
    given = ranks if ranks is not None else fractions
    K = len(given)
    if not (1 <= K <= abi.SELECT_MAX_RANKS):
        raise ValueError(f"{K} ranks: a select takes 1 .. {abi.SELECT_MAX_RANKS}")
    if ranks is not None:
        for k in ranks:
            if not (1 <= int(k) < (1 << 64)):
                raise ValueError(f"rank {k} must be >= 1 and fit the ABI's u64")
        return np.asarray([int(k) for k in ranks], dtype=np.uint64), None
    fr = np.ascontiguousarray(fractions, dtype=np.float64)
    if not np.all((fr > 0.0) & (fr <= 1.0)):
        raise ValueError("every fraction must be in (0, 1]")
    return None, fr


def _target_hists(targets, hist_bins: int) -> np.ndarray:
    """`targets` as the ABI's [P][hist_bins] u64 histograms."""
    tgt = np.ascontiguousarray(targets, dtype=np.uint64)
    if tgt.ndim != 2 or tgt.shape[1] != hist_bins:
        raise ValueError("targets must be [P][hist_bins]: one histogram of hist_bins entries per target")
    return tgt


def _threshold_rows(thresholds) -> np.ndarray:
    """`thresholds` as the ABI's [Q][4] f64 rows."""
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    if thr.ndim != 2 or thr.shape[1] != 4:
        raise ValueError("thresholds must be [Q][4]: ks, mean_rel, entropy_rel, frequency_diff per row")
    return thr


def _digit_arrays(pass_: int, prefixes):
    """The checked `prefixes` [4][K] u64 of one pass of a select, and the [4][K][256] u64 array the pass fills."""
    pre = np.ascontiguousarray(prefixes, dtype=np.uint64)
    if pre.ndim != 2 or pre.shape[0] != 4 or not (1 <= pre.shape[1] <= abi.SELECT_MAX_RANKS):
        raise ValueError(f"prefixes must be [4][K], K in 1 .. {abi.SELECT_MAX_RANKS}")
    if not (0 <= int(pass_) < abi.SELECT_PASSES):
        raise ValueError(f"pass_ = {pass_} must be in 0 .. {abi.SELECT_PASSES - 1}")
    return pre, np.zeros((4, pre.shape[1], 256), dtype=np.uint64)


def _select_result(K: int, name: str, call) -> SelectResult:
    """A select's outputs, filled by call(out_population, out_ranks, out_values, out_counts_le): the last four
    arguments of both select calls."""
    population = C.c_uint64()
    out_ranks = np.zeros(K, dtype=np.uint64)
    values = np.zeros((4, K), dtype=np.float64)
    counts_le = np.zeros((4, K), dtype=np.uint64)
    _check(call(C.byref(population), out_ranks.ctypes.data, values.ctypes.data, counts_le.ctypes.data), name)
    return SelectResult(int(population.value), out_ranks, values, counts_le)


class Context:
    """A device-resident run (ecdna_ssa_ctx): create once, launch many times."""

    def __init__(self, spec: "abi.RunSpec", ext: Optional["abi.Ext"] = None,
                 passages: Optional["abi.Passages"] = None, cohort: Optional["abi.Cohort"] = None,
                 keep: Optional["abi.Keep"] = None, keep_timepoints: Optional["abi.KeepTimepoints"] = None):
        """`ext`: an explicit extension block (ecdna_ssa_ctx_create_ext); default: the one `spec` asks for, if any.
        `passages`: likewise the passage block (ecdna_ssa_ctx_create_passages), `cohort`: the cohort block
        (ecdna_ssa_ctx_create_cohort), `keep`: the keep block (ecdna_ssa_ctx_create_keep), `keep_timepoints`: the
        timepoint keep block (ecdna_ssa_ctx_create_keep_timepoints)."""
        self.spec = spec
        self.params = spec.params()
        self.ext = ext if ext is not None else spec.ext()
        self.passages = passages if passages is not None else spec.passages()
        self.cohort = cohort if cohort is not None else spec.cohort()
        self.keep = keep if keep is not None else spec.keep()
        self.keep_timepoints = keep_timepoints if keep_timepoints is not None else spec.keep_timepoints()
        self._rescore_targets = 0
        h = C.c_void_p()

        def ref(block):
            return C.byref(block) if block is not None else None

        if self.keep_timepoints is not None:  # (only a spec that asks for them goes through _keep_timepoints)
            _check(self._keep_timepoints_lib().ecdna_ssa_ctx_create_keep_timepoints(
                C.byref(self.params), ref(self.ext), ref(self.passages), ref(self.cohort), ref(self.keep),
                C.byref(self.keep_timepoints), C.byref(h)), "ecdna_ssa_ctx_create_keep_timepoints")
        elif self.keep is not None:  # (only a spec that asks for kept samples goes through _keep)
            _check(self._keep_lib().ecdna_ssa_ctx_create_keep(
                C.byref(self.params), ref(self.ext), ref(self.passages), ref(self.cohort), C.byref(self.keep),
                C.byref(h)), "ecdna_ssa_ctx_create_keep")
        elif self.cohort is not None:  # (only a spec that asks for a cohort goes through _cohort)
            _check(_lib_with("ecdna_ssa_ctx_create_cohort").ecdna_ssa_ctx_create_cohort(
                C.byref(self.params), ref(self.ext), ref(self.passages), C.byref(self.cohort), C.byref(h)),
                "ecdna_ssa_ctx_create_cohort")
        elif self.passages is not None:  # (only a spec that asks for passages goes through _passages)
            _check(_lib_with("ecdna_ssa_ctx_create_passages").ecdna_ssa_ctx_create_passages(
                C.byref(self.params), ref(self.ext), C.byref(self.passages), C.byref(h)),
                "ecdna_ssa_ctx_create_passages")
        elif self.ext is not None:  # (only a spec that asks for the extension goes through _ext)
            _check(_lib_with("ecdna_ssa_ctx_create_ext").ecdna_ssa_ctx_create_ext(
                C.byref(self.params), C.byref(self.ext), C.byref(h)), "ecdna_ssa_ctx_create_ext")
        else:
            _check(lib().ecdna_ssa_ctx_create(C.byref(self.params), C.byref(h)), "ecdna_ssa_ctx_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().ecdna_ssa_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_outputs(self, d_hist: int = 0, d_totals: int = 0):
        _check(lib().ecdna_ssa_ctx_set_outputs(self.h, d_hist or None, d_totals or None), "set_outputs")

    def launch(self, stream: int = 0):
        _check(lib().ecdna_ssa_ctx_launch(self.h, stream or None), "ecdna_ssa_ctx_launch")

    def sync(self):
        s, hh = C.c_float(), C.c_float()
        _check(lib().ecdna_ssa_ctx_sync(self.h, C.byref(s), C.byref(hh)), "ecdna_ssa_ctx_sync")
        return s.value, hh.value

    def reduce(self, comm: "Comm"):
        """All-reduce (sum) this context's histogram and totals over `comm` on its launch stream (RCCL)."""
        _check(lib().ecdna_ssa_ctx_reduce(self.h, comm.h), "ecdna_ssa_ctx_reduce")

    def geometry(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().ecdna_ssa_ctx_geometry(self.h, C.byref(a), C.byref(b)), "geometry")
        return a.value, b.value

    def instance(self) -> dict:
        """The kernel instance this context launches (schedule, pairing, rotation, K, VGPRs, ...): ABI v7."""
        ins = abi.Instance()
        _check(lib().ecdna_ssa_ctx_instance(self.h, C.byref(ins)), "instance")
        return ins.as_dict()

    def row_stride(self) -> int:
        return int(lib().ecdna_ssa_ctx_row_stride(self.h))

    def accept_timepoints(self, source: int) -> int:
        """T of an acceptance source: 1, the spec's snapshots, its passages, its cohort's targets, or the targets of
        the last rescore; for the rescored timepoints, the context's snapshots or passages."""
        if source == abi.ACCEPT_RESCORED:
            return self._rescore_targets
        if source == abi.ACCEPT_RESCORED_TIMEPOINTS:
            return self.timepoints()
        if source in (abi.ACCEPT_COHORT, abi.ACCEPT_COHORT_SAMPLES):
            return int(self.cohort.n_targets) if self.cohort is not None else 0
        if source in (abi.ACCEPT_SNAPSHOTS, abi.ACCEPT_SNAPSHOT_SAMPLES):
            return int(self.params.n_snapshots)
        if source in (abi.ACCEPT_PASSAGES, abi.ACCEPT_PASSAGE_SAMPLES):
            return int(self.passages.n_passages) if self.passages is not None else 0
        return 1

    def accept_enqueue(self, source: int, thresholds, timepoints=None, list_threshold: int = 0,
                       list_capacity: int = 0):
        """Enqueue the acceptance pass on the stream of the last launch (ecdna_ssa_ctx_accept); download_accept
        returns its results. Arguments as accept()."""
        _lib_with("ecdna_ssa_ctx_accept")
        thr = _threshold_rows(thresholds)
        mask = timepoint_mask(timepoints)
        for name, v, bits in (("list_threshold", list_threshold, 32), ("list_capacity", list_capacity, 64),
                              ("source", source, 32), ("n_thresholds", thr.shape[0], 32)):
            if not (0 <= int(v) < (1 << bits)):
                raise ValueError(f"{name} = {v} does not fit the ABI's u{bits} field")
        a = abi.Accept(struct_size=C.sizeof(abi.Accept), source=int(source), n_thresholds=thr.shape[0],
                       list_threshold=int(list_threshold), timepoint_mask=mask, list_capacity=int(list_capacity))
        a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
        self._accept_shape = None
        _check(lib().ecdna_ssa_ctx_accept(self.h, C.byref(a)), "ecdna_ssa_ctx_accept")
        self._accept_shape = (thr.shape[0], self.accept_timepoints(int(source)),
                              min(int(list_capacity), int(self.params.n_replicates)))

    def download_accept(self) -> AcceptResult:
        """The results of the last accept_enqueue (ecdna_ssa_ctx_download_accept; synchronises)."""
        shape = getattr(self, "_accept_shape", None)
        if shape is None:
            raise EngineError("download_accept before accept")
        Q, T, cap = shape
        p = self.params
        counts = np.zeros((Q, p.n_param_sets), dtype=np.uint64)
        mask = np.zeros(p.n_replicates, dtype=np.uint32)
        ids = np.zeros(cap, dtype=np.uint64)
        stats = np.zeros((cap, T), dtype=abi.STATS_DTYPE)
        n_acc = C.c_uint64()
        _check(lib().ecdna_ssa_ctx_download_accept(self.h, counts.ctypes.data, mask.ctypes.data, C.byref(n_acc),
                                                   ids.ctypes.data if cap else None,
                                                   stats.ctypes.data if cap else None), "ecdna_ssa_ctx_download_accept")
        listed = min(int(n_acc.value), cap)
        return AcceptResult(counts, mask, int(n_acc.value), ids[:listed], stats[:listed])

    def accept(self, source: int, thresholds, timepoints=None, list_threshold: int = 0,
               list_capacity: int = 0) -> AcceptResult:
        """ABC rejection on the GPU over the statistics of the last launch (acceptance mapping v1): `source` an
        abi.ACCEPT_* constant; `thresholds` array-like [Q][4] in the order ks, mean_rel, entropy_rel, frequency_diff
        (np.inf switches a statistic off); `timepoints` an iterable of the indices that take part (None: all);
        the replicates accepted under row `list_threshold` are listed, at most `list_capacity` of them. May be called
        any number of times after one launch."""
        self.accept_enqueue(source, thresholds, timepoints, list_threshold, list_capacity)
        return self.download_accept()

    def accept_draws_enqueue(self, targets, sample_cells, thresholds, n_draws: int = 64, first_draw: int = 0,
                             timepoints=None, store: str = "keep"):
        """Enqueue the acceptance over thinning draws first_draw .. first_draw + n_draws - 1 on the stream of the last
        launch (ecdna_ssa_ctx_accept_draws); download_accept_draws returns its results. Arguments as accept_draws()."""
        L = _lib_with("ecdna_ssa_ctx_accept_draws")
        a, _alive = self._accept_draws_block(targets, sample_cells, thresholds, n_draws, first_draw, timepoints, store)
        self._accept_draws_shape = None
        _check(L.ecdna_ssa_ctx_accept_draws(self.h, C.byref(a)), "ecdna_ssa_ctx_accept_draws")
        self._accept_draws_shape = (int(a.n_thresholds), int(n_draws))

    def _accept_draws_block(self, targets, sample_cells, thresholds, n_draws, first_draw, timepoints, store):
        """The block ecdna_ssa_accept_draws_t of accept_draws' arguments, and the arrays it points into. thresholds
        None: a block without threshold rows, as select_draws takes it."""
        if store not in ("keep", "timepoints"):
            raise ValueError('store must be "keep" or "timepoints"')
        tgt = _target_hists(targets, self.params.hist_bins)
        thr = _threshold_rows(thresholds if thresholds is not None else np.zeros((0, 4)))
        for name, v in (("n_targets", tgt.shape[0]), ("n_thresholds", thr.shape[0]), ("n_draws", n_draws),
                        ("first_draw", first_draw)):
            _check_u32(name, v)
        cells = self._u32_list("sample_cells", sample_cells, tgt.shape[0])
        a = abi.AcceptDraws(struct_size=C.sizeof(abi.AcceptDraws), timepoints=int(store == "timepoints"),
                            n_targets=tgt.shape[0], first_draw=int(first_draw), n_draws=int(n_draws),
                            n_thresholds=thr.shape[0], timepoint_mask=timepoint_mask(timepoints))
        a.target_hists = tgt.ctypes.data_as(C.POINTER(C.c_uint64))
        a.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
        if thresholds is not None:
            a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
        return a, (tgt, cells, thr)

    def download_accept_draws(self) -> AcceptDrawsResult:
        """The results of the last accept_draws_enqueue (ecdna_ssa_ctx_download_accept_draws; synchronises)."""
        shape = getattr(self, "_accept_draws_shape", None)
        if shape is None:
            raise EngineError("download_accept_draws before accept_draws")
        Q, n_draws = shape
        p = self.params
        sums = np.zeros((Q, p.n_param_sets), dtype=np.uint64)
        passes = np.zeros((p.n_replicates, Q), dtype=np.uint8)
        _check(lib().ecdna_ssa_ctx_download_accept_draws(self.h, sums.ctypes.data,
                                                         passes.ctypes.data if passes.size else None),
               "ecdna_ssa_ctx_download_accept_draws")
        return AcceptDrawsResult(sums, passes, n_draws)

    def accept_draws(self, targets, sample_cells, thresholds, n_draws: int = 64, first_draw: int = 0, timepoints=None,
                     store: str = "keep") -> AcceptDrawsResult:
        """Acceptance over repeated thinnings of the kept samples (thinned acceptance mapping v1): for every replicate
        and row of `thresholds` [Q][4], on how many of the thinning draws first_draw .. first_draw + n_draws - 1 the
        replicate is accepted when target p is scored on sample_cells[p] of its kept cells — what rescore(targets,
        sample_cells, [d] * P) and accept(ACCEPT_RESCORED, ...) give, summed over d, in one pass that stores no record.
        store "keep": `targets` [P][hist_bins] against the kept sample, `timepoints` names the participating targets
        (None: all, jointly); "timepoints": one target per timepoint of the timepoint keep block, as
        rescore_timepoints and ACCEPT_RESCORED_TIMEPOINTS. The rescored records, accept's results and select's keys are
        left as they are."""
        self.accept_draws_enqueue(targets, sample_cells, thresholds, n_draws, first_draw, timepoints, store)
        return self.download_accept_draws()

    def pool_draws(self, targets, sample_cells, thresholds, threshold: int = 0, n_draws: int = 64, first_draw: int = 0,
                   timepoints=None, store: str = "keep") -> PoolDrawsResult:
        """The accepted thinnings pooled (ecdna_ssa_ctx_pool_draws, thinned pooling mapping v1): the arguments of
        accept_draws() and one row `threshold` of `thresholds`. Per global parameter set, .thinned[slot] sums the
        histograms of the thinned samples of sample_cells[slot] cells over the replicates and the draws that pass the
        row — every slot, those `timepoints` leaves out of the verdict included — and .kept[slice] the whole kept
        samples times the number of passing draws (one slice on store "keep", T on "timepoints"). Synchronous; needs
        neither an earlier accept_draws nor a rescore and leaves their results as they are."""
        L = _lib_with("ecdna_ssa_ctx_pool_draws")
        a, _alive = self._accept_draws_block(targets, sample_cells, thresholds, n_draws, first_draw, timepoints, store)
        _check_u32("threshold", threshold)
        if int(threshold) >= int(a.n_thresholds):
            raise ValueError(f"threshold = {threshold} must be a row of thresholds, < {int(a.n_thresholds)}")
        p = self.params
        slices = int(a.n_targets) if store == "timepoints" else 1
        thinned = np.zeros((int(a.n_targets), p.n_param_sets, p.hist_bins), dtype=np.uint64)
        kept = np.zeros((slices, p.n_param_sets, p.hist_bins), dtype=np.uint64)
        _check(L.ecdna_ssa_ctx_pool_draws(self.h, C.byref(a), int(threshold), thinned.ctypes.data, kept.ctypes.data),
               "ecdna_ssa_ctx_pool_draws")
        return PoolDrawsResult(thinned, kept)

    def select(self, source: int, ranks=None, fractions=None, timepoints=None) -> SelectResult:
        """ABC thresholds on the GPU (ecdna_ssa_ctx_select, select mapping v1): the exact `ranks`-th smallest values
        (ranks >= 1), or those at `fractions` in (0, 1] of the population, of each of the four distances among the
        error-free replicates of `source` (an abi.ACCEPT_* constant), the maximum over `timepoints` (None: all) standing
        for a replicate. accept() with a finite value as the one threshold accepts exactly its counts_le replicates."""
        _lib_with("ecdna_ssa_ctx_select")
        rk, fr = select_ranks(ranks, fractions)
        _check_u32("source", source)
        K = len(rk) if rk is not None else len(fr)
        s = abi.Select(struct_size=C.sizeof(abi.Select), source=int(source), timepoint_mask=timepoint_mask(timepoints),
                       n_ranks=K)
        if rk is not None:
            s.ranks = rk.ctypes.data_as(C.POINTER(C.c_uint64))
        else:
            s.fractions = fr.ctypes.data_as(C.POINTER(C.c_double))
        return _select_result(K, "ecdna_ssa_ctx_select",
                              lambda *out: lib().ecdna_ssa_ctx_select(self.h, C.byref(s), *out))

    def select_digits(self, source: int, pass_: int, prefixes, timepoints=None) -> np.ndarray:
        """One pass of the select on this context's replicates (ecdna_ssa_ctx_select_digits), the shard primitive:
        `prefixes` [4][K] u64 keys (shard.SelectWalk.prefixes), the result [4][K][256] u64: per distance and prefix, the
        population's keys that share the prefix's top 8 * pass_ bits, counted by their next 8 bits. Shards' arrays sum."""
        _lib_with("ecdna_ssa_ctx_select_digits")
        pre, hist = _digit_arrays(pass_, prefixes)
        _check_u32("source", source)
        _check(lib().ecdna_ssa_ctx_select_digits(self.h, int(source), timepoint_mask(timepoints), int(pass_),
                                                 pre.shape[1], pre.ctypes.data, hist.ctypes.data),
               "ecdna_ssa_ctx_select_digits")
        return hist

    def select_draws(self, targets, sample_cells, n_draws: int = 64, first_draw: int = 0, timepoints=None,
                     store: str = "keep", ranks=None, fractions=None) -> SelectResult:
        """ABC thresholds over thinning draws (ecdna_ssa_ctx_select_draws, thinned select mapping v1): select()'s order
        statistics over the pairs (error-free replicate, thinning draw) of accept_draws()' arguments without thresholds —
        the population is (error-free replicates) x n_draws, and a pair's key the maximum over the participating slots of
        the distance accept_draws scores on that draw. accept_draws() with a finite value as its one threshold has
        sums[0].sum() == counts_le. Synchronous; stores no record, needs no rescore and leaves the rescored records and
        the results of accept, accept_draws and select as they are."""
        L = _lib_with("ecdna_ssa_ctx_select_draws")
        rk, fr = select_ranks(ranks, fractions)
        K = len(rk) if rk is not None else len(fr)
        a, _alive = self._accept_draws_block(targets, sample_cells, None, n_draws, first_draw, timepoints, store)
        return _select_result(K, "ecdna_ssa_ctx_select_draws", lambda *out: L.ecdna_ssa_ctx_select_draws(
            self.h, C.byref(a), K, rk.ctypes.data if rk is not None else None,
            fr.ctypes.data if fr is not None else None, *out))

    def select_draws_digits(self, targets, sample_cells, pass_: int, prefixes, n_draws: int = 64, first_draw: int = 0,
                            timepoints=None, store: str = "keep") -> np.ndarray:
        """One pass of select_draws on this context's replicates (ecdna_ssa_ctx_select_draws_digits), the shard
        primitive: select_digits() over the keys of every (replicate, draw). Pass 0 makes the keys; the later passes
        read them and must name the same block. Shards' arrays sum."""
        L = _lib_with("ecdna_ssa_ctx_select_draws_digits")
        pre, hist = _digit_arrays(pass_, prefixes)
        a, _alive = self._accept_draws_block(targets, sample_cells, None, n_draws, first_draw, timepoints, store)
        _check(L.ecdna_ssa_ctx_select_draws_digits(self.h, C.byref(a), int(pass_), pre.shape[1], pre.ctypes.data,
                                                   hist.ctypes.data), "ecdna_ssa_ctx_select_draws_digits")
        return hist

    def download_cohort(self) -> CohortResult:
        """The cohort records of the last launch (ecdna_ssa_ctx_download_cohort): stats and sample_stats [P][n]."""
        _lib_with("ecdna_ssa_ctx_download_cohort")
        if self.cohort is None:  # (the library refuses: ECDNA_E_STATE)
            _check(lib().ecdna_ssa_ctx_download_cohort(self.h, None, None), "ecdna_ssa_ctx_download_cohort")
            raise EngineError("ecdna_ssa_ctx_download_cohort: the context has no cohort block")
        P_, n = int(self.cohort.n_targets), int(self.params.n_replicates)
        st = np.zeros((P_, n), dtype=abi.STATS_DTYPE)
        sst = np.zeros((P_, n), dtype=abi.STATS_DTYPE) if self.cohort.sample_cells else None
        _check(lib().ecdna_ssa_ctx_download_cohort(self.h, st.ctypes.data, sst.ctypes.data if sst is not None else None),
               "ecdna_ssa_ctx_download_cohort")
        return CohortResult(st, sst)

    # What the calls of the keep block and their twins of the timepoint keep block share: the library with the block's
    # entry points, a pooled histogram with a leading axis of T slices, and a download of kept samples with the leading
    # axes `lead` (none, or T).
    @staticmethod
    def _keep_lib():
        return _lib_with("ecdna_ssa_ctx_create_keep")

    @staticmethod
    def _keep_timepoints_lib():
        return _lib_with("ecdna_ssa_ctx_create_keep_timepoints")

    def _pool_accepted(self, get_lib, name: str, T: int, threshold: int) -> np.ndarray:
        _check_u32("threshold", threshold)
        p = self.params
        out = np.zeros((max(T, 1), p.n_param_sets, p.hist_bins), dtype=np.uint64)
        _check(getattr(get_lib(), name)(self.h, int(threshold), out.ctypes.data), name)
        return out[:T]

    def _download_kept(self, get_lib, name: str, lead: tuple, m: int, ids, count):
        if ids is not None:
            if count is not None:
                raise ValueError("give ids or count, not both")
            idv = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
            k = len(idv)
        else:
            idv = None
            k = int(self.params.n_replicates) if count is None else int(count)
            if not (0 <= k < (1 << 64)):
                raise ValueError(f"count = {count} does not fit the ABI's u64 field")
        headers = np.zeros(lead + (k,), dtype=abi.KEPT_DTYPE)
        cells = np.zeros(lead + (k, m), dtype=np.uint16)
        _check(getattr(get_lib(), name)(self.h, k, idv.ctypes.data if idv is not None and k else None,
                                        headers.ctypes.data if headers.size else None,
                                        cells.ctypes.data if cells.size else None), name)
        return headers, cells

    @staticmethod
    def _sized_lib():
        return _lib_with("ecdna_ssa_ctx_rescore_sized")

    @staticmethod
    def _u32_list(name: str, values, count: int) -> np.ndarray:
        """`values` (one number for all, or one per target) as the ABI's [count] u32 array."""
        arr = np.asarray(values)
        if arr.ndim == 0:
            arr = np.full(count, arr)
        if arr.shape != (count,):
            raise ValueError(f"{name} must be one number, or one per target ({count})")
        if arr.size and not (np.issubdtype(arr.dtype, np.integer) and arr.min() >= 0 and arr.max() < (1 << 32)):
            raise ValueError(f"{name} does not fit the ABI's u32 fields")
        return np.ascontiguousarray(arr, dtype=np.uint32)

    def rescore_enqueue(self, targets, sample_cells=None, draws=None):
        """Enqueue the late scoring of the kept samples against `targets` [P][hist_bins] on the stream of the last
        launch (ecdna_ssa_ctx_rescore; with sample_cells or draws, ecdna_ssa_ctx_rescore_sized); download_rescored
        returns the records."""
        tgt = _target_hists(targets, self.params.hist_bins)
        if not (0 <= tgt.shape[0] < (1 << 32)):
            raise ValueError(f"{tgt.shape[0]} targets do not fit the ABI's u32 field")
        self._rescore_targets = 0
        if sample_cells is None and draws is None:
            _check(self._keep_lib().ecdna_ssa_ctx_rescore(self.h, tgt.shape[0], tgt.ctypes.data),
                   "ecdna_ssa_ctx_rescore")
        else:
            cells = None if sample_cells is None else self._u32_list("sample_cells", sample_cells, tgt.shape[0])
            dr = None if draws is None else self._u32_list("draws", draws, tgt.shape[0])
            r = abi.Rescore(struct_size=C.sizeof(abi.Rescore), n_targets=tgt.shape[0])
            r.target_hists = tgt.ctypes.data_as(C.POINTER(C.c_uint64))
            if cells is not None:
                r.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
            if dr is not None:
                r.sample_draws = dr.ctypes.data_as(C.POINTER(C.c_uint32))
            _check(self._sized_lib().ecdna_ssa_ctx_rescore_sized(self.h, C.byref(r)), "ecdna_ssa_ctx_rescore_sized")
        self._rescore_targets = tgt.shape[0]

    def download_rescored(self) -> np.ndarray:
        """The records of the last rescore, [P][n] abi.STATS_DTYPE (ecdna_ssa_ctx_download_rescored; synchronises)."""
        out = np.zeros((self._rescore_targets, int(self.params.n_replicates)), dtype=abi.STATS_DTYPE)
        _check(self._keep_lib().ecdna_ssa_ctx_download_rescored(self.h, out.ctypes.data if out.size else None),
               "ecdna_ssa_ctx_download_rescored")
        return out

    def rescore(self, targets, sample_cells=None, draws=None) -> np.ndarray:
        """Score every replicate's kept sample (RunSpec.keep_cells) against targets that need not have been known at
        create: records [P][n] abi.STATS_DTYPE, byte for byte those of a run with stats_target = targets[p] and
        subsample_cells = keep_cells. They are the acceptance source abi.ACCEPT_RESCORED until the next rescore or
        launch.
        sample_cells (one number, or one per target, each 1 .. keep_cells): target p is scored on a uniform sample of
        sample_cells[p] of the kept cells instead — the law of having measured that many cells (thinning mapping v1) —
        and draws (each 0 .. 63) picks one of 64 independent such thinnings per target."""
        self.rescore_enqueue(targets, sample_cells, draws)
        return self.download_rescored()

    def pool_accepted(self, threshold: int) -> np.ndarray:
        """The posterior predictive histogram (ecdna_ssa_ctx_pool_accepted): per global parameter set, the sum of the
        kept samples' histograms of the replicates the last accept() accepted under row `threshold`,
        [n_param_sets][hist_bins] u64. Shards' arrays sum to the whole run's."""
        return self._pool_accepted(self._keep_lib, "ecdna_ssa_ctx_pool_accepted", 1, threshold)[0]

    def download_kept(self, ids=None, count: Optional[int] = None):
        """Kept samples of the last launch (ecdna_ssa_ctx_download_kept): (headers [k] abi.KEPT_DTYPE, cells
        [k][keep_cells] u16) of the replicates with the global `ids`, in their order (an AcceptResult's ids as they
        come), or of the call's first `count` replicates (default: all). cells[j][:headers[j]["nplus"]] are the N+
        cells' true copy numbers, ascending; the rest of a row is unspecified."""
        m = int(self.keep.keep_cells) if self.keep is not None else 0
        return self._download_kept(self._keep_lib, "ecdna_ssa_ctx_download_kept", (), m, ids, count)

    def timepoints(self) -> int:
        """T of the timepoint keep block: the context's growth phases, else its snapshots with snapshot statistics."""
        if self.passages is not None:
            return int(self.passages.n_passages)
        if self.ext is not None and self.ext.snapshot_stats:
            return int(self.params.n_snapshots)
        return 0

    def _kept_timepoints(self) -> int:
        return self.timepoints() if self.keep_timepoints is not None else 0

    def rescore_timepoints_enqueue(self, targets, sample_cells=None, draw: int = 0):
        """Enqueue the late scoring of the kept timepoint samples against one longitudinal target, `targets`
        [T][hist_bins], on the stream of the last launch (ecdna_ssa_ctx_rescore_timepoints; with sample_cells,
        ecdna_ssa_ctx_rescore_timepoints_sized); download_rescored_timepoints returns the records."""
        tgt = np.ascontiguousarray(targets, dtype=np.uint64)
        if self.keep_timepoints is not None and (tgt.ndim != 2 or tgt.shape != (self.timepoints(), self.params.hist_bins)):
            raise ValueError("targets must be [T][hist_bins]: one histogram of hist_bins entries per timepoint")
        if sample_cells is None and draw == 0:
            _check(self._keep_timepoints_lib().ecdna_ssa_ctx_rescore_timepoints(self.h, tgt.ctypes.data if tgt.size else None),
                   "ecdna_ssa_ctx_rescore_timepoints")
            return
        _check_u32("draw", draw)
        # (a context without the block: the library says so, whatever the sizes' shape)
        count = self.timepoints() if self.keep_timepoints is not None else int(np.size(sample_cells))
        cells = None if sample_cells is None else self._u32_list("sample_cells", sample_cells, count)
        _check(self._sized_lib().ecdna_ssa_ctx_rescore_timepoints_sized(
            self.h, tgt.ctypes.data if tgt.size else None, cells.ctypes.data if cells is not None and cells.size else None,
            int(draw)), "ecdna_ssa_ctx_rescore_timepoints_sized")

    def download_rescored_timepoints(self) -> np.ndarray:
        """The records of the last rescore_timepoints, [T][n] abi.STATS_DTYPE
        (ecdna_ssa_ctx_download_rescored_timepoints; synchronises)."""
        out = np.zeros((self._kept_timepoints(), int(self.params.n_replicates)), dtype=abi.STATS_DTYPE)
        _check(self._keep_timepoints_lib().ecdna_ssa_ctx_download_rescored_timepoints(
            self.h, out.ctypes.data if out.size else None), "ecdna_ssa_ctx_download_rescored_timepoints")
        return out

    def rescore_timepoints(self, targets, sample_cells=None, draw: int = 0) -> np.ndarray:
        """Score every replicate's kept sample of every timepoint (RunSpec.keep_timepoint_cells) against a longitudinal
        target that need not have been known at create: records [T][n] abi.STATS_DTYPE, byte for byte the sample
        records of a run created with these targets as passage_targets (or as snapshot_targets with
        snapshot_subsample_cells = keep_timepoint_cells). They are the acceptance source
        abi.ACCEPT_RESCORED_TIMEPOINTS until the next rescore_timepoints or launch.
        sample_cells (one number, or one per timepoint, each 1 .. keep_timepoint_cells): timepoint t is scored on a
        uniform sample of sample_cells[t] of its kept cells instead (thinning mapping v1), on thinning `draw` (0 .. 63)."""
        self.rescore_timepoints_enqueue(targets, sample_cells, draw)
        return self.download_rescored_timepoints()

    def pool_accepted_timepoints(self, threshold: int) -> np.ndarray:
        """The posterior predictive histogram per timepoint (ecdna_ssa_ctx_pool_accepted_timepoints): per timepoint and
        global parameter set, the sum of the kept samples' histograms of the replicates the last accept() accepted
        under row `threshold`, [T][n_param_sets][hist_bins] u64. Shards' arrays sum to the whole run's."""
        return self._pool_accepted(self._keep_timepoints_lib, "ecdna_ssa_ctx_pool_accepted_timepoints",
                                   self._kept_timepoints(), threshold)

    def download_kept_timepoints(self, ids=None, count: Optional[int] = None):
        """Kept timepoint samples of the last launch (ecdna_ssa_ctx_download_kept_timepoints): (headers [T][k]
        abi.KEPT_DTYPE, cells [T][k][keep_timepoint_cells] u16) of the replicates with the global `ids`, in their order,
        or of the call's first `count` replicates (default: all). cells[t][j][:headers[t][j]["nplus"]] are the N+
        cells' true copy numbers, ascending; the rest of a row is unspecified."""
        m = int(self.keep_timepoints.keep_cells) if self.keep_timepoints is not None else 0
        return self._download_kept(self._keep_timepoints_lib, "ecdna_ssa_ctx_download_kept_timepoints",
                                   (self._kept_timepoints(),), m, ids, count)

    def download(self, want_rows: bool = False) -> Result:
        p = self.params
        summ = abi.summaries_array(p.n_replicates)
        hist = np.zeros(p.n_param_sets * p.hist_bins, dtype=np.uint64)
        tot = abi.totals_array(p.n_param_sets)
        rows = None
        stride = 0
        if want_rows:
            stride = self.row_stride()
            if stride <= 0:
                raise EngineError("rows are not downloadable from a chunked run")
            rows = np.zeros((p.n_replicates, stride), dtype=np.uint16)
        _check(lib().ecdna_ssa_ctx_download(self.h, summ.ctypes.data, hist.ctypes.data, tot.ctypes.data,
                                            rows.ctypes.data if rows is not None else None), "download")
        res = Result(summ, hist.reshape(p.n_param_sets, p.hist_bins), tot, rows, stride)
        if p.n_snapshots:
            S = p.n_snapshots
            meta = np.zeros((p.n_replicates, S), dtype=abi.SNAPSHOT_DTYPE)
            srows = None
            if p.flags & abi.FLAG_SNAPSHOT_ROWS:
                st = (p.cell_cap + 63) // 64 * 64  # snapshot rows always use the 128-B aligned stride
                srows = np.zeros((p.n_replicates, S, st), dtype=np.uint16)
            _check(lib().ecdna_ssa_ctx_download_snapshots(self.h, meta.ctypes.data,
                                                          srows.ctypes.data if srows is not None else None),
                   "download_snapshots")
            res.snapshots = meta
            res.snapshot_rows = srows
        if p.flags & abi.FLAG_REP_STATS:
            st = np.zeros(p.n_replicates, dtype=abi.STATS_DTYPE)
            _check(lib().ecdna_ssa_ctx_download_stats(self.h, st.ctypes.data), "download_stats")
            res.stats = st
        if p.subsample_cells or self.passages is not None:  # (a passage run: the last phase's sample)
            st = np.zeros(p.n_replicates, dtype=abi.STATS_DTYPE)
            sh = np.zeros(p.n_param_sets * p.hist_bins, dtype=np.uint64)
            _check(lib().ecdna_ssa_ctx_download_sample(self.h, st.ctypes.data, sh.ctypes.data), "download_sample")
            res.sample_stats = st
            res.sample_hist = sh.reshape(p.n_param_sets, p.hist_bins)
        if self.ext is not None and self.ext.snapshot_stats:
            S, m = p.n_snapshots, self.ext.snapshot_subsample_cells
            shape = (S, p.n_param_sets, p.hist_bins)
            st = np.zeros((p.n_replicates, S), dtype=abi.STATS_DTYPE)
            sh = np.zeros(shape, dtype=np.uint64)
            sst = np.zeros((p.n_replicates, S), dtype=abi.STATS_DTYPE) if m else None
            ssh = np.zeros(shape, dtype=np.uint64) if m else None
            _check(lib().ecdna_ssa_ctx_download_snapshot_stats(
                self.h, st.ctypes.data, sst.ctypes.data if m else None, sh.ctypes.data, ssh.ctypes.data if m else None),
                "download_snapshot_stats")
            res.snapshot_stats, res.snapshot_hist = st, sh
            res.snapshot_sample_stats, res.snapshot_sample_hist = sst, ssh
        if self.passages is not None:
            G, n, sets = self.passages.n_passages, p.n_replicates, p.n_param_sets
            out = PassageResult(np.zeros((G, n), dtype=abi.SUMMARY_DTYPE), np.zeros((G, sets), dtype=abi.TOTALS_DTYPE),
                                np.zeros((G, n), dtype=abi.STATS_DTYPE), np.zeros((G, n), dtype=abi.STATS_DTYPE),
                                np.zeros((G, sets, p.hist_bins), dtype=np.uint64),
                                np.zeros((G, sets, p.hist_bins), dtype=np.uint64))
            _check(lib().ecdna_ssa_ctx_download_passages(
                self.h, out.summaries.ctypes.data, out.totals.ctypes.data, out.stats.ctypes.data,
                out.sample_stats.ctypes.data, out.hist.ctypes.data, out.sample_hist.ctypes.data), "download_passages")
            res.passages = out
        if self.cohort is not None:
            res.cohort = self.download_cohort()
        if p.flags & abi.FLAG_REFERENCE_DRAWS:
            w = np.zeros(p.n_replicates, dtype=np.uint64)
            _check(lib().ecdna_ssa_ctx_download_rng_words(self.h, w.ctypes.data), "download_rng_words")
            res.rng_words = w
        return res


def run(spec: "abi.RunSpec", want_rows: bool = False) -> Result:
    """Run every replicate of `spec` on device `spec.device` and return host copies of the results."""
    with Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        return ctx.download(want_rows=want_rows)
