"""ABC thresholds over thinning draws (ecdna_ssa_ctx_select_draws and _select_draws_digits, added within ABI v13; thinned
select mapping v1) without a GPU: the header declares the two calls, the library exports them, the
ctypes argtypes match, the version is still 13 and the older blocks kept their sizes, the header states the mapping and
its contracts, and without a context the calls answer ECDNA_E_INVALID."""
import ctypes as C
import re

import numpy as np

from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9
NEW_CALLS = ("ecdna_ssa_ctx_select_draws", "ecdna_ssa_ctx_select_draws_digits")


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_select_draws") == [
        "ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a", "uint32_t n_ranks", "const uint64_t* ranks",
        "const double* fractions", "uint64_t* out_population", "uint64_t* out_ranks", "double* out_values",
        "uint64_t* out_counts_le"]
    assert declared("ecdna_ssa_ctx_select_draws_digits") == [
        "ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a", "uint32_t pass", "uint32_t n_prefixes",
        "const uint64_t* prefixes", "uint64_t* out_hist"]
    # the calls they stand beside did not change
    assert declared("ecdna_ssa_ctx_accept_draws") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a"]
    assert declared("ecdna_ssa_ctx_pool_draws") == [
        "ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a", "uint32_t threshold", "uint64_t* out_thinned",
        "uint64_t* out_kept"]
    assert declared("ecdna_ssa_ctx_select_digits") == [
        "ecdna_ssa_ctx* c", "uint32_t source", "uint64_t timepoint_mask", "uint32_t pass", "uint32_t n_prefixes",
        "const uint64_t* prefixes", "uint64_t* out_hist"]
    for name in NEW_CALLS:
        assert hasattr(product_lib, name) and name in engine.EXPORTS, name
    P = C.POINTER
    assert product_lib.ecdna_ssa_ctx_select_draws.argtypes == [
        C.c_void_p, P(abi.AcceptDraws), C.c_uint32, C.c_void_p, C.c_void_p, P(C.c_uint64), C.c_void_p, C.c_void_p,
        C.c_void_p] == abi.SELECT_DRAWS_ARGTYPES
    assert product_lib.ecdna_ssa_ctx_select_draws_digits.argtypes == [
        C.c_void_p, P(abi.AcceptDraws), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p] == abi.SELECT_DRAWS_DIGITS_ARGTYPES
    assert product_lib.ecdna_ssa_ctx_select_draws.restype == product_lib.ecdna_ssa_ctx_select_draws_digits.restype == C.c_int
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_the_older_blocks_kept_their_sizes(tmp_path):
    got = layout(tmp_path, {"accept_draws": "ecdna_ssa_accept_draws_t", "accept": "ecdna_ssa_accept_t",
                            "threshold": "ecdna_accept_threshold_t", "select": "ecdna_ssa_select_t",
                            "rescore": "ecdna_ssa_rescore_t", "keep": "ecdna_ssa_keep_t",
                            "keep_timepoints": "ecdna_ssa_keep_timepoints_t", "cohort": "ecdna_ssa_cohort_t",
                            "stats": "ecdna_rep_stats_t", "params": "ecdna_ssa_params_t"})
    assert got["accept_draws"] == C.sizeof(abi.AcceptDraws) == 72
    assert got["accept"] == C.sizeof(abi.Accept) == 48 and got["threshold"] == C.sizeof(abi.AcceptThreshold) == 32
    assert got["select"] == C.sizeof(abi.Select) == 40 and got["rescore"] == C.sizeof(abi.Rescore) == 40
    assert got["keep"] == C.sizeof(abi.Keep) == 16 and got["keep_timepoints"] == C.sizeof(abi.KeepTimepoints) == 16
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32 and got["stats"] == abi.STATS_DTYPE.itemsize == 64
    assert got["params"] == C.sizeof(abi.Params)


def _block(hists, cells):
    a = abi.AcceptDraws(struct_size=C.sizeof(abi.AcceptDraws), n_targets=hists.shape[0], n_draws=64)
    a.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    a.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
    return a


def test_null_context_is_invalid(product_lib):
    hists = np.ones((1, BINS), dtype=np.uint64)
    cells = np.asarray([5], dtype=np.uint32)
    fr = np.asarray([0.5])
    pre = np.zeros((4, 1), dtype=np.uint64)
    hist = np.zeros((4, 1, 256), dtype=np.uint64)
    a = _block(hists, cells)
    assert product_lib.ecdna_ssa_ctx_select_draws(None, C.byref(a), 1, None, fr.ctypes.data, None, None, None,
                                                  None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_select_draws(None, None, 1, None, fr.ctypes.data, None, None, None,
                                                  None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_select_draws_digits(None, C.byref(a), 0, 1, pre.ctypes.data,
                                                         hist.ctypes.data) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_select_draws_digits(None, None, 0, 1, None, None) == abi.E_INVALID


def test_a_keep_context_before_a_launch(product_lib):
    """A keep context where there is a device, ECDNA_E_NODEVICE where there is none — and then the calls on it: a bad
    block or bad ranks are ECDNA_E_INVALID first, good ones ECDNA_E_STATE before a launch."""
    spec = abi.RunSpec(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_cells=20)
    p, k, h = spec.params(), spec.keep(), C.c_void_p()
    rc = product_lib.ecdna_ssa_ctx_create_keep(C.byref(p), None, None, None, C.byref(k), C.byref(h))
    assert rc in (abi.OK, abi.E_NODEVICE)
    if rc != abi.OK:
        return
    try:
        hists = np.ones((2, BINS), dtype=np.uint64)
        cells = np.asarray([20, 21], dtype=np.uint32)
        fr = np.asarray([0.5])
        call = lambda a, K=1: product_lib.ecdna_ssa_ctx_select_draws(h, C.byref(a), K, None, fr.ctypes.data, None, None,
                                                                     None, None)
        assert call(_block(hists, cells)) == abi.E_INVALID
        assert b"sample_cells[1]" in product_lib.ecdna_ssa_last_error_message()
        cells[1] = 7
        assert call(_block(hists, cells), 0) == abi.E_INVALID
        assert b"select_draws.n_ranks" in product_lib.ecdna_ssa_last_error_message()
        a = _block(hists, cells)
        a.n_thresholds = 1
        assert call(a) == abi.E_INVALID
        assert b"select_draws.n_thresholds" in product_lib.ecdna_ssa_last_error_message()
        assert call(_block(hists, cells)) == abi.E_STATE
    finally:
        product_lib.ecdna_ssa_ctx_destroy(h)


def test_the_header_states_thinned_select_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Thinned select mapping v1",
                   "the population a quantile cuts is the pseudo-datasets, the pairs (replicate, draw)",
                   "n_thresholds must be 0 and thresholds NULL",
                   "n_replicates x n_draws must be below 2^32",
                   "M = (error-free replicates) x n_draws",
                   "on a passage context the rule per participating phase",
                   "key_x(i, d) is the maximum, over the participating slots",
                   "the same f64 operations in the same order",
                   "the same whole-sample rule when m1 >= a + b (one record, counted on every draw)",
                   "the key of 0.0",
                   "Nothing of thinning mapping v1 or of thinned acceptance mapping v1 changes",
                   "over-rank (value +inf, counts_le = M)",
                   "Ranks are u64; M can reach 2^32",
                   "S1. ecdna_ssa_ctx_select_draws_digits(block, pass, prefixes) equals the sum, over the draws d of the "
                   "range",
                   "S2. For a finite value_x(k), ecdna_ssa_ctx_accept_draws with the same block and one row",
                   "no smaller threshold reaches k",
                   "S3. With n_draws = 1 the four outputs are bit for bit those of ecdna_ssa_ctx_select",
                   "S4. Shards' digit arrays sum to the whole run's. Nothing depends on chunk, shard, grid or device",
                   "32 x n x n_draws bytes: 2.1 GB at n = 2^20 and 64 draws",
                   "pass 0 of the same block must come first",
                   "They need no earlier rescore"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): ABC " \
           "thresholds over thinning draws" in text
