"""The kept samples of every timepoint (ecdna_ssa_keep_timepoints_t, added within ABI v13; timepoint keep mapping v1,
DESIGN.md §3.4) without a GPU: the header declares the block, its create call, the four calls over the kept samples and
the acceptance source 13, the library exports the calls, the ctypes mirror has the header's layout, the version is
still 13 and the older blocks kept their sizes, the header states the mapping, ecdna_ssa_ctx_create_keep_timepoints
validates the block before any device is touched, and RunSpec builds it."""
import ctypes as C
import re

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9
NEW_CALLS = ("ecdna_ssa_ctx_create_keep_timepoints", "ecdna_ssa_ctx_rescore_timepoints",
             "ecdna_ssa_ctx_download_rescored_timepoints", "ecdna_ssa_ctx_pool_accepted_timepoints",
             "ecdna_ssa_ctx_download_kept_timepoints")


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_create_keep_timepoints") == [
        "const ecdna_ssa_params_t* p", "const ecdna_ssa_ext_t* ext", "const ecdna_ssa_passages_t* passages",
        "const ecdna_ssa_cohort_t* cohort", "const ecdna_ssa_keep_t* keep",
        "const ecdna_ssa_keep_timepoints_t* keep_timepoints", "ecdna_ssa_ctx** out"]
    assert declared("ecdna_ssa_ctx_rescore_timepoints") == ["ecdna_ssa_ctx* c", "const uint64_t* target_hists"]
    assert declared("ecdna_ssa_ctx_download_rescored_timepoints") == ["ecdna_ssa_ctx* c", "ecdna_rep_stats_t* out"]
    assert declared("ecdna_ssa_ctx_pool_accepted_timepoints") == [
        "ecdna_ssa_ctx* c", "uint32_t threshold", "uint64_t* out_hist"]
    assert declared("ecdna_ssa_ctx_download_kept_timepoints") == [
        "ecdna_ssa_ctx* c", "uint64_t n_ids", "const uint64_t* ids", "ecdna_kept_t* out_headers", "uint16_t* out_cells"]
    for name in NEW_CALLS:
        assert hasattr(product_lib, name) and name in engine.EXPORTS, name
    # additive: the version is v13's, and the keep block's create call is still declared as it was
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13
    assert declared("ecdna_ssa_ctx_create_keep")[-2:] == ["const ecdna_ssa_keep_t* keep", "ecdna_ssa_ctx** out"]


def test_null_context_calls_are_invalid(product_lib):
    hists = np.ones((2, BINS), dtype=np.uint64)
    out = np.zeros(2 * BINS, dtype=np.uint64)
    assert product_lib.ecdna_ssa_ctx_rescore_timepoints(None, hists.ctypes.data) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_download_rescored_timepoints(None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_pool_accepted_timepoints(None, 0, out.ctypes.data) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_download_kept_timepoints(None, 0, None, None, None) == abi.E_INVALID


def test_the_header_states_timepoint_keep_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Timepoint keep mapping v1",
                   "Replicate ids are global",
                   "the sample that snapshot_subsample_cells = m defines for that pair, unchanged",
                   "\"nminus N- cells, then the snapshot row\"",
                   "stream field (s + 1) << 16 under the run's key",
                   "ext->snapshot_subsample_cells keeps its meaning and stays independent of the block",
                   "A snapshot that was not taken keeps {0, 0}",
                   "keep_cells must equal passage_cells",
                   "phase g's sample under seed_g, stream field 0",
                   "are the founders of phase g + 1",
                   "The last phase is kept too",
                   "an ECDNA_REP_ERR_EMPTY phase is one",
                   "nminus + nplus = min(m, N)",
                   "{0xffffffff, 0xffffffff} for a sample the guard ended",
                   "headers[T][n] and cells[T][n][m]",
                   "T × n × (2m + 8) bytes",
                   "arithmetic, not a measurement",
                   "Nothing depends on chunk, shard, grid or device. Chunked runs are covered",
                   "with or without ECDNA_FLAG_SNAPSHOT_ROWS",
                   "out_sample_stats[t][i] of the same run created with passage_target_hists = target_hists",
                   "out_sample_stats[i][t] of the same run created with snapshot_target_hists = target_hists and "
                   "snapshot_subsample_cells = m",
                   "drops the keys ecdna_ssa_ctx_select cached",
                   "a relaunch invalidates them",
                   "ECDNA_ACCEPT_RESCORED_TIMEPOINTS = 13",
                   "rep stride 1, timepoint stride n",
                   "every participating phase error-free",
                   "the one-summary rule of ECDNA_ACCEPT_FINAL",
                   "the message names ecdna_ssa_ctx_create_keep_timepoints",
                   "shards' arrays sum to the whole run's",
                   "The five older create calls forward to this one"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): the sample " \
           "of every timepoint of a longitudinal run kept on the GPU" in text


def test_layout_and_source_match_header(tmp_path):
    """sizeof, the field offsets and the source's value from a compiled C probe against the ctypes mirror; the older
    blocks and sources did not move."""
    fields = [f for f, _ in abi.KeepTimepoints._fields_]
    assert fields == ["struct_size", "keep_cells", "reserved"]
    got = layout(tmp_path, {"kt": ("ecdna_ssa_keep_timepoints_t", fields), "keep": "ecdna_ssa_keep_t",
                            "kept": "ecdna_kept_t", "cohort": "ecdna_ssa_cohort_t", "accept": "ecdna_ssa_accept_t",
                            "select": "ecdna_ssa_select_t", "passages": "ecdna_ssa_passages_t", "ext": "ecdna_ssa_ext_t",
                            "instance": "ecdna_ssa_instance_t", "params": "ecdna_ssa_params_t"},
                 values={"source": "ECDNA_ACCEPT_RESCORED_TIMEPOINTS", "rescored": "ECDNA_ACCEPT_RESCORED",
                         "cohort_samples": "ECDNA_ACCEPT_COHORT_SAMPLES",
                         "passage_samples": "ECDNA_ACCEPT_PASSAGE_SAMPLES"})
    assert got["kt"] == C.sizeof(abi.KeepTimepoints) == 16
    for f in fields:
        assert got[f"kt.{f}"] == getattr(abi.KeepTimepoints, f).offset, f
    assert got["source"] == abi.ACCEPT_RESCORED_TIMEPOINTS == 13
    assert got["rescored"] == abi.ACCEPT_RESCORED == 12 and got["cohort_samples"] == 9 and got["passage_samples"] == 5
    assert got["keep"] == C.sizeof(abi.Keep) == 16 and got["kept"] == C.sizeof(abi.Kept) == 8
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32 and got["accept"] == C.sizeof(abi.Accept) == 48
    assert got["select"] == C.sizeof(abi.Select) == 40
    assert got["passages"] == C.sizeof(abi.Passages) == 24 and got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["instance"] == C.sizeof(abi.Instance) and got["params"] == C.sizeof(abi.Params) == 184


SNAP = dict(snapshots=(2, 10), snapshot_stats=True)
PAS = dict(n_passages=2, passage_cells=20)


def _spec(**kw):
    base = dict(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_timepoint_cells=20)
    base.update(kw)
    return abi.RunSpec(**base)


def _create(lib, spec, kt, keep=None):
    def ref(block):
        return C.byref(block) if block is not None else None

    p = spec.params()
    ext, pas, co = spec.ext(), spec.passages(), spec.cohort()
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create_keep_timepoints(C.byref(p), ref(ext), ref(pas), ref(co), ref(keep), ref(kt), C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_rejects_bad_blocks(product_lib):
    """Before any device is touched: E_INVALID with a message that names the field, GPU or not."""
    for kind in (SNAP, PAS):
        s = _spec(**kind)
        for size in (0, C.sizeof(abi.KeepTimepoints) - 4, C.sizeof(abi.KeepTimepoints) + 8):
            b = s.keep_timepoints()
            b.struct_size = size
            rc, msg = _create(product_lib, s, b)
            assert rc == abi.E_INVALID and "keep_timepoints.struct_size" in msg, (kind, size)
        for r in (1, 1 << 40):
            b = s.keep_timepoints()
            b.reserved = r
            rc, msg = _create(product_lib, s, b)
            assert rc == abi.E_INVALID and "keep_timepoints.reserved" in msg, (kind, r)
        for m in (0, 4097, (1 << 32) - 1):
            s1 = _spec(keep_timepoint_cells=m, **kind)
            rc, msg = _create(product_lib, s1, s1.keep_timepoints())
            assert rc == abi.E_INVALID and "keep_timepoints.keep_cells" in msg, (kind, m)
        s2 = _spec(flags=0, **kind)
        rc, msg = _create(product_lib, s2, s2.keep_timepoints())
        assert rc == abi.E_INVALID and "REP_STATS" in msg, kind
    # neither a passage block nor snapshot_stats: an ordinary run, and snapshots without their statistics
    for kw in (dict(), dict(snapshots=(2, 10))):
        s3 = _spec(**kw)
        rc, msg = _create(product_lib, s3, s3.keep_timepoints())
        assert rc == abi.E_INVALID and "passages" in msg and "snapshot_stats" in msg, kw
    # a passage block with another sample size
    for m in (19, 21, 1, 4096):
        s4 = _spec(keep_timepoint_cells=m, **PAS)
        rc, msg = _create(product_lib, s4, s4.keep_timepoints())
        assert rc == abi.E_INVALID and "keep_cells" in msg and "passage_cells" in msg, m
    # a parameter error of the params themselves, and of another block, is still reported through the new call
    s5 = _spec(hist_bins=1, **SNAP)
    rc, msg = _create(product_lib, s5, s5.keep_timepoints())
    assert rc == abi.E_INVALID and "hist_bins" in msg
    s6 = _spec(keep_cells=0, **SNAP)
    rc, msg = _create(product_lib, s6, s6.keep_timepoints(), keep=s6.keep())
    assert rc == abi.E_INVALID and "keep.keep_cells" in msg
    # the end-of-run keep block still refuses a passage block, in its own words
    s7 = _spec(keep_cells=20, **PAS)
    rc, msg = _create(product_lib, s7, s7.keep_timepoints(), keep=s7.keep())
    assert rc == abi.E_INVALID and "every phase" in msg


def test_create_accepts_good_blocks(product_lib):
    """In range: whatever comes back (no device here, a context there), it is not a parameter error."""
    for kw in (SNAP, PAS, dict(keep_timepoint_cells=1, **SNAP), dict(keep_timepoint_cells=4096, **SNAP),
               dict(keep_timepoint_cells=65, **SNAP),
               dict(keep_timepoint_cells=1, n_passages=3, passage_cells=1),
               dict(keep_timepoint_cells=4096, n_passages=2, passage_cells=4096, max_cells=5000),
               dict(snapshot_subsample_cells=7, **SNAP),  # stays independent of the block
               dict(flags=abi.FLAG_REP_STATS | abi.FLAG_SNAPSHOT_ROWS, **SNAP),
               dict(passage_targets=np.ones((2, BINS), dtype=np.uint64), **PAS)):
        s = _spec(**kw)
        rc, msg = _create(product_lib, s, s.keep_timepoints())
        assert rc in (abi.OK, abi.E_NODEVICE), (kw, rc, msg)
    # the end-of-run keep block beside a snapshot context stays legal and independent
    s = _spec(keep_cells=33, **SNAP)
    rc, msg = _create(product_lib, s, s.keep_timepoints(), keep=s.keep())
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    # keep_timepoints == NULL: exactly ecdna_ssa_ctx_create_keep, whose checks still run
    off = _spec(keep_timepoint_cells=None, flags=0)
    assert off.keep_timepoints() is None
    rc, msg = _create(product_lib, off, None)
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    bad = _spec(keep_timepoint_cells=None, keep_cells=4097)
    rc, msg = _create(product_lib, bad, None, keep=bad.keep())
    assert rc == abi.E_INVALID and "keep_cells" in msg


def test_runspec_builds_the_block():
    b = _spec(**SNAP).keep_timepoints()
    assert b.struct_size == C.sizeof(abi.KeepTimepoints) == 16 and b.keep_cells == 20 and b.reserved == 0
    assert abi.RunSpec().keep_timepoints() is None and abi.RunSpec().keep_timepoint_cells is None
    assert _spec(keep_timepoint_cells=0).keep_timepoints().keep_cells == 0  # (a block the library refuses)
    assert _spec(**SNAP).timepoints() == 2 and _spec(**PAS).timepoints() == 2
    assert _spec().timepoints() == 0 and _spec(snapshots=(2, 10)).timepoints() == 0
    with pytest.raises(ValueError):
        _spec(keep_timepoint_cells=1 << 32).keep_timepoints()
    with pytest.raises(ValueError):
        _spec(keep_timepoint_cells=-1).keep_timepoints()
