"""The sized rescore (ecdna_ssa_rescore_t, ecdna_ssa_ctx_rescore_sized and _rescore_timepoints_sized, added within ABI
v13; thinning mapping v1) without a GPU: the header declares the block and the two calls, the library
exports them, the ctypes mirror has the header's layout, the version is still 13 and the older blocks kept their sizes,
the header states the mapping, and without a context the calls answer as their siblings do."""
import ctypes as C
import re

import numpy as np

from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9
NEW_CALLS = ("ecdna_ssa_ctx_rescore_sized", "ecdna_ssa_ctx_rescore_timepoints_sized")


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_rescore_sized") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_rescore_t* r"]
    assert declared("ecdna_ssa_ctx_rescore_timepoints_sized") == [
        "ecdna_ssa_ctx* c", "const uint64_t* target_hists", "const uint32_t* sample_cells", "uint32_t draw"]
    # the unsized calls did not change
    assert declared("ecdna_ssa_ctx_rescore") == [
        "ecdna_ssa_ctx* c", "uint32_t n_targets", "const uint64_t* target_hists"]
    assert declared("ecdna_ssa_ctx_rescore_timepoints") == ["ecdna_ssa_ctx* c", "const uint64_t* target_hists"]
    for name in NEW_CALLS:
        assert hasattr(product_lib, name) and name in engine.EXPORTS, name
    assert product_lib.ecdna_ssa_ctx_rescore_sized.argtypes == [C.c_void_p, C.POINTER(abi.Rescore)]
    assert product_lib.ecdna_ssa_ctx_rescore_timepoints_sized.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p,
                                                                           C.c_uint32]
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror; the older blocks did not move."""
    fields = [f for f, _ in abi.Rescore._fields_]
    assert fields == ["struct_size", "n_targets", "target_hists", "sample_cells", "sample_draws", "reserved"]
    got = layout(tmp_path, {"rescore": ("ecdna_ssa_rescore_t", fields), "keep": "ecdna_ssa_keep_t",
                            "keep_timepoints": "ecdna_ssa_keep_timepoints_t", "cohort": "ecdna_ssa_cohort_t",
                            "stats": "ecdna_rep_stats_t", "params": "ecdna_ssa_params_t"},
                 values={"rescored_source": "ECDNA_ACCEPT_RESCORED",
                         "rescored_timepoints_source": "ECDNA_ACCEPT_RESCORED_TIMEPOINTS"})
    assert got["rescore"] == C.sizeof(abi.Rescore) == 40
    for f in fields:
        assert got[f"rescore.{f}"] == getattr(abi.Rescore, f).offset, f
    assert got["keep"] == C.sizeof(abi.Keep) == 16 and got["keep_timepoints"] == C.sizeof(abi.KeepTimepoints) == 16
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32 and got["stats"] == abi.STATS_DTYPE.itemsize == 64
    assert (got["rescored_source"], got["rescored_timepoints_source"]) == (12, 13)
    assert got["params"] == C.sizeof(abi.Params)
    assert abi.THIN_MAX_DRAW == 63


def _block(hists, cells=None, draws=None):
    r = abi.Rescore(struct_size=C.sizeof(abi.Rescore), n_targets=hists.shape[0])
    r.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    if cells is not None:
        r.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
    if draws is not None:
        r.sample_draws = draws.ctypes.data_as(C.POINTER(C.c_uint32))
    return r


def test_null_arguments_are_invalid_as_the_siblings_are(product_lib):
    """Without a context (and so without a GPU) the new calls answer what ecdna_ssa_ctx_rescore and
    _rescore_timepoints answer."""
    hists = np.ones((1, BINS), dtype=np.uint64)
    cells = np.asarray([5], dtype=np.uint32)
    r = _block(hists, cells)
    sibling = product_lib.ecdna_ssa_ctx_rescore(None, 1, hists.ctypes.data)
    assert product_lib.ecdna_ssa_ctx_rescore_sized(None, C.byref(r)) == sibling == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_rescore_sized(None, None) == abi.E_INVALID
    sibling = product_lib.ecdna_ssa_ctx_rescore_timepoints(None, hists.ctypes.data)
    assert product_lib.ecdna_ssa_ctx_rescore_timepoints_sized(None, hists.ctypes.data, cells.ctypes.data,
                                                              0) == sibling == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_rescore_timepoints_sized(None, None, None, 64) == abi.E_INVALID


def test_a_context_answers_as_its_siblings_do(product_lib):
    """A keep context where there is a device, ECDNA_E_NODEVICE where there is none — and then the calls on it: before a
    launch both the sized call and its sibling say ECDNA_E_STATE, and a bad block is ECDNA_E_INVALID first."""
    spec = abi.RunSpec(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_cells=20)
    p, k, h = spec.params(), spec.keep(), C.c_void_p()
    rc = product_lib.ecdna_ssa_ctx_create_keep(C.byref(p), None, None, None, C.byref(k), C.byref(h))
    assert rc in (abi.OK, abi.E_NODEVICE)
    if rc != abi.OK:
        return
    try:
        hists = np.ones((2, BINS), dtype=np.uint64)
        cells = np.asarray([20, 21], dtype=np.uint32)
        assert product_lib.ecdna_ssa_ctx_rescore_sized(h, C.byref(_block(hists, cells))) == abi.E_INVALID
        assert b"sample_cells[1]" in product_lib.ecdna_ssa_last_error_message()
        cells[1] = 7
        sibling = product_lib.ecdna_ssa_ctx_rescore(h, 2, hists.ctypes.data)
        assert product_lib.ecdna_ssa_ctx_rescore_sized(h, C.byref(_block(hists, cells))) == sibling == abi.E_STATE
        sibling = product_lib.ecdna_ssa_ctx_rescore_timepoints(h, hists.ctypes.data)
        assert product_lib.ecdna_ssa_ctx_rescore_timepoints_sized(h, hists.ctypes.data, cells.ctypes.data,
                                                                  0) == sibling == abi.E_STATE
    finally:
        product_lib.ecdna_ssa_ctx_destroy(h)


def test_the_header_states_thinning_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Thinning mapping v1",
                   "A uniform m1-subset of a uniform m-subset of a population is a uniform m1-subset of that population",
                   "A header {0xffffffff, 0xffffffff} gives the all-zero record for every target",
                   "positions 0 .. a - 1 are N- cells (k = 0), position a + j is cells[j]",
                   "A target with m1 >= N_k is scored on the whole kept sample",
                   "subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above) is applied unchanged to this "
                   "population with N = N_k and m = m1",
                   "the run's seed, or seed_g for growth phase g of a passage context",
                   "counter word 1 is base_tau | 0x20000000 | (d << 10) | t, t < 2^10 the block index",
                   "0xC0000000 for the end of the run and for passage phases, 0xC0000000 | (s + 1) << 16 for snapshot s",
                   "d in 0 .. 63",
                   "t takes bits 0-9, d bits 10-15, the snapshot field bits 16-22, the thinning flag bit 29, the tag "
                   "bits 30-31",
                   "No existing stream has bits 29, 30 and 31 all set",
                   "Targets with equal (m1, d) see the same thinned sample",
                   "Nothing depends on chunk, shard, grid or device",
                   "NOT byte for byte a relaunch with subsample_cells = m1",
                   "It has the same law",
                   "still pool and return the whole kept samples",
                   "byte for byte the unsized call's",
                   "a target with more measured cells than were kept cannot be served honestly"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): the kept " \
           "samples rescored at each target's own number of measured cells" in text
