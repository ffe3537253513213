"""Acceptance over repeated thinnings (ecdna_ssa_accept_draws_t, ecdna_ssa_ctx_accept_draws and
_download_accept_draws, added within ABI v13; thinned acceptance mapping v1) without a GPU: the header
declares the block and the two calls, the library exports them, the ctypes mirror has the header's layout, the version is
still 13 and the older blocks kept their sizes, the header states the mapping, and without a context the calls answer as
ecdna_ssa_ctx_accept does."""
import ctypes as C
import re

import numpy as np

from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9
NEW_CALLS = ("ecdna_ssa_ctx_accept_draws", "ecdna_ssa_ctx_download_accept_draws")
FIELDS = ["struct_size", "timepoints", "n_targets", "target_hists", "sample_cells", "first_draw", "n_draws",
          "n_thresholds", "thresholds", "timepoint_mask", "reserved"]


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_accept_draws") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a"]
    assert declared("ecdna_ssa_ctx_download_accept_draws") == [
        "ecdna_ssa_ctx* c", "uint64_t* out_sums", "uint8_t* out_passes"]
    # the calls it stands beside did not change
    assert declared("ecdna_ssa_ctx_accept") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_t* a"]
    assert declared("ecdna_ssa_ctx_rescore_sized") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_rescore_t* r"]
    for name in NEW_CALLS:
        assert hasattr(product_lib, name) and name in engine.EXPORTS, name
    assert product_lib.ecdna_ssa_ctx_accept_draws.argtypes == [C.c_void_p, C.POINTER(abi.AcceptDraws)]
    assert product_lib.ecdna_ssa_ctx_download_accept_draws.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror; the older blocks did not move."""
    assert [f for f, _ in abi.AcceptDraws._fields_] == FIELDS
    got = layout(tmp_path, {"accept_draws": ("ecdna_ssa_accept_draws_t", FIELDS), "accept": "ecdna_ssa_accept_t",
                            "threshold": "ecdna_accept_threshold_t", "select": "ecdna_ssa_select_t",
                            "rescore": "ecdna_ssa_rescore_t", "keep": "ecdna_ssa_keep_t",
                            "keep_timepoints": "ecdna_ssa_keep_timepoints_t", "cohort": "ecdna_ssa_cohort_t",
                            "stats": "ecdna_rep_stats_t", "params": "ecdna_ssa_params_t"})
    assert got["accept_draws"] == C.sizeof(abi.AcceptDraws) == 72
    for f in FIELDS:
        assert got[f"accept_draws.{f}"] == getattr(abi.AcceptDraws, f).offset, f
    assert got["accept"] == C.sizeof(abi.Accept) == 48 and got["threshold"] == C.sizeof(abi.AcceptThreshold) == 32
    assert got["select"] == C.sizeof(abi.Select) == 40 and got["rescore"] == C.sizeof(abi.Rescore) == 40
    assert got["keep"] == C.sizeof(abi.Keep) == 16 and got["keep_timepoints"] == C.sizeof(abi.KeepTimepoints) == 16
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32 and got["stats"] == abi.STATS_DTYPE.itemsize == 64
    assert got["params"] == C.sizeof(abi.Params)
    assert abi.ACCEPT_DRAWS_MAX == abi.THIN_MAX_DRAW + 1 == 64


def _block(hists, cells, thr):
    a = abi.AcceptDraws(struct_size=C.sizeof(abi.AcceptDraws), n_targets=hists.shape[0], n_draws=64,
                        n_thresholds=thr.shape[0])
    a.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    a.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
    a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
    return a


def test_null_arguments_are_invalid_as_accept_says(product_lib):
    """Without a context (and so without a GPU) the new calls answer what ecdna_ssa_ctx_accept answers."""
    hists = np.ones((1, BINS), dtype=np.uint64)
    cells = np.asarray([5], dtype=np.uint32)
    thr = np.full((1, 4), np.inf)
    sibling_block = abi.Accept(struct_size=C.sizeof(abi.Accept), source=abi.ACCEPT_RESCORED, n_thresholds=1)
    sibling_block.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
    sibling = product_lib.ecdna_ssa_ctx_accept(None, C.byref(sibling_block))
    assert product_lib.ecdna_ssa_ctx_accept_draws(None, C.byref(_block(hists, cells, thr))) == sibling == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_accept_draws(None, None) == abi.E_INVALID
    sibling = product_lib.ecdna_ssa_ctx_download_accept(None, None, None, None, None, None)
    assert product_lib.ecdna_ssa_ctx_download_accept_draws(None, None, None) == sibling == abi.E_INVALID


def test_a_keep_context_before_a_launch(product_lib):
    """A keep context where there is a device, ECDNA_E_NODEVICE where there is none — and then the call on it: a bad block
    is ECDNA_E_INVALID first, a good one ECDNA_E_STATE before a launch, as the download is."""
    spec = abi.RunSpec(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_cells=20)
    p, k, h = spec.params(), spec.keep(), C.c_void_p()
    rc = product_lib.ecdna_ssa_ctx_create_keep(C.byref(p), None, None, None, C.byref(k), C.byref(h))
    assert rc in (abi.OK, abi.E_NODEVICE)
    if rc != abi.OK:
        return
    try:
        hists = np.ones((2, BINS), dtype=np.uint64)
        cells = np.asarray([20, 21], dtype=np.uint32)
        thr = np.full((1, 4), np.inf)
        assert product_lib.ecdna_ssa_ctx_accept_draws(h, C.byref(_block(hists, cells, thr))) == abi.E_INVALID
        assert b"sample_cells[1]" in product_lib.ecdna_ssa_last_error_message()
        cells[1] = 7
        assert product_lib.ecdna_ssa_ctx_accept_draws(h, C.byref(_block(hists, cells, thr))) == abi.E_STATE
        assert product_lib.ecdna_ssa_ctx_download_accept_draws(h, None, None) == abi.E_STATE
    finally:
        product_lib.ecdna_ssa_ctx_destroy(h)


def test_the_header_states_thinned_acceptance_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Thinned acceptance mapping v1",
                   "the share of them a replicate passes estimates its acceptance probability under measurement noise",
                   "a draw range first_draw .. first_draw + n_draws - 1 inside 0 .. 63",
                   "n_targets = P in 1 .. 64 targets for the same slice",
                   "exactly one target per timepoint (n_targets == T), as for source 13",
                   "every target is scored on the thinned sample that thinning mapping v1 defines for "
                   "(sample_cells[slot], d)",
                   "the same key per slice (seed, or seed_g), the same stream tag, the same grouping",
                   "the same whole-sample rule when m1 >= a + b, the same guard records",
                   "Replicate i passes row q on draw d iff acceptance mapping v1 accepts it on those records",
                   "on a passage context: per participating phase",
                   "A tie passes, +inf switches a statistic off, a NaN fails",
                   "passes[i][q], u8, laid out [n][Q]",
                   "sums[Q][n_param_sets], u64: per row and GLOBAL parameter set",
                   "shards' arrays sum to the whole run's",
                   "That equality is part of the contract",
                   "the same f64 operations in the same order",
                   "It needs no earlier rescore",
                   "a later call replaces the results, a relaunch invalidates them"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): acceptance " \
           "over repeated thinnings of the kept samples" in text
