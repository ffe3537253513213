"""The kept samples (ecdna_ssa_keep_t, added within ABI v13; keep mapping v1) without a GPU: the header
declares the block, its create call, the four calls over the kept samples and the acceptance source 12, the library
exports the calls, the ctypes mirrors have the header's layout, the version is still 13 and the older blocks kept their
sizes, the header states the mapping, ecdna_ssa_ctx_create_keep validates the block before any device is touched, and
RunSpec builds it."""
import ctypes as C
import re

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.abi import HEADER, PARAMS_SIZE_V13, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9
NEW_CALLS = ("ecdna_ssa_ctx_create_keep", "ecdna_ssa_ctx_rescore", "ecdna_ssa_ctx_download_rescored",
             "ecdna_ssa_ctx_pool_accepted", "ecdna_ssa_ctx_download_kept")


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_create_keep") == [
        "const ecdna_ssa_params_t* p", "const ecdna_ssa_ext_t* ext", "const ecdna_ssa_passages_t* passages",
        "const ecdna_ssa_cohort_t* cohort", "const ecdna_ssa_keep_t* keep", "ecdna_ssa_ctx** out"]
    assert declared("ecdna_ssa_ctx_rescore") == [
        "ecdna_ssa_ctx* c", "uint32_t n_targets", "const uint64_t* target_hists"]
    assert declared("ecdna_ssa_ctx_download_rescored") == ["ecdna_ssa_ctx* c", "ecdna_rep_stats_t* out"]
    assert declared("ecdna_ssa_ctx_pool_accepted") == [
        "ecdna_ssa_ctx* c", "uint32_t threshold", "uint64_t* out_hist"]
    assert declared("ecdna_ssa_ctx_download_kept") == [
        "ecdna_ssa_ctx* c", "uint64_t n_ids", "const uint64_t* ids", "ecdna_kept_t* out_headers", "uint16_t* out_cells"]
    for name in NEW_CALLS:
        assert hasattr(product_lib, name) and name in engine.EXPORTS, name
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_null_context_calls_are_invalid(product_lib):
    hists = np.ones((1, BINS), dtype=np.uint64)
    out = np.zeros(BINS, dtype=np.uint64)
    assert product_lib.ecdna_ssa_ctx_rescore(None, 1, hists.ctypes.data) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_download_rescored(None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_pool_accepted(None, 0, out.ctypes.data) == abi.E_INVALID
    assert product_lib.ecdna_ssa_ctx_download_kept(None, 0, None, None, None) == abi.E_INVALID


def test_the_source_is_12():
    text = header_text()
    assert re.search(r"\bECDNA_ACCEPT_RESCORED\s*=\s*12\b", text) and abi.ACCEPT_RESCORED == 12
    assert re.search(r"\bECDNA_ACCEPT_COHORT_SAMPLES\s*=\s*9\s*,", text)  # the older ones did not move
    assert re.search(r"\bECDNA_ACCEPT_COHORT\s*=\s*8\s*,", text)
    assert (abi.ACCEPT_FINAL, abi.ACCEPT_PASSAGE_SAMPLES, abi.ACCEPT_COHORT, abi.ACCEPT_COHORT_SAMPLES) == (0, 5, 8, 9)
    # 6, 7, 10 and 11 name nothing
    assert not re.search(r"\bECDNA_ACCEPT_\w+\s*=\s*(6|7|10|11)\b", text)
    values = sorted(int(v) for v in re.findall(r"\bECDNA_ACCEPT_\w+\s*=\s*(\d+)", text))
    assert values == [0, 1, 2, 3, 4, 5, 8, 9, 12]


def test_the_header_states_keep_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Keep mapping v1",
                   "the sample that subsample mapping v1",
                   "stream field 0, counter (i, 0xC0000000 | t, r lo, r hi), the run's key, r the GLOBAL id",
                   "the same sample that subsample_cells = m, and a cohort target with sample_cells[p] = m, see",
                   "nminus + nplus = min(m, N)",
                   "TRUE copy numbers (not the clipped bins), ascending: the founder format of passage mapping v1",
                   "Entries past nplus are unspecified",
                   "An extinct or never-started replicate keeps the empty sample {0, 0}",
                   "A sample the guard ended keeps {0xffffffff, 0xffffffff}",
                   "rescored as the all-zero record",
                   "does not depend on chunk, shard, grid or device. Chunked runs are covered",
                   "kept samples of every phase are a different feature",
                   "byte for byte the record ecdna_ssa_ctx_download_sample returns for the same run with "
                   "stats_target_hist = target_hists[p] and subsample_cells = keep_cells",
                   "drops the keys ecdna_ssa_ctx_select cached, as a relaunch does",
                   "a relaunch invalidates the records",
                   "T = the P of the last rescore, timepoint p is target p",
                   "the one-summary rule of ECDNA_ACCEPT_FINAL",
                   "rep stride 1, timepoint stride n, error stride 0",
                   "10 and 11 are not sources",
                   "bin 0 holds the N- cells, true copy numbers are clipped at hist_bins - 1",
                   "shards' arrays sum to the whole run's",
                   "it takes ecdna_ssa_ctx_download_accept's out_ids as they come",
                   "The four older create calls forward to this one"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): every " \
           "replicate's sample kept on the GPU" in text


def test_keep_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirrors; the older blocks did not move."""
    keep_fields = [f for f, _ in abi.Keep._fields_]
    kept_fields = [f for f, _ in abi.Kept._fields_]
    assert keep_fields == ["struct_size", "keep_cells", "reserved"] and kept_fields == ["nminus", "nplus"]
    got = layout(tmp_path, {"keep": ("ecdna_ssa_keep_t", keep_fields), "kept": ("ecdna_kept_t", kept_fields),
                            "cohort": ("ecdna_ssa_cohort_t", ["reserved"]), "select": "ecdna_ssa_select_t",
                            "accept": ("ecdna_ssa_accept_t", ["reserved"]), "passages": "ecdna_ssa_passages_t",
                            "ext": "ecdna_ssa_ext_t", "stats": "ecdna_rep_stats_t", "summary": "ecdna_rep_summary_t",
                            "instance": "ecdna_ssa_instance_t", "params": ("ecdna_ssa_params_t", ["subsample_cells"])},
                 values={"rescored_source": "ECDNA_ACCEPT_RESCORED",
                         "cohort_samples_source": "ECDNA_ACCEPT_COHORT_SAMPLES"})
    assert got["keep"] == C.sizeof(abi.Keep) == 16 and got["kept"] == C.sizeof(abi.Kept) == abi.KEPT_DTYPE.itemsize == 8
    for f in keep_fields:
        assert got[f"keep.{f}"] == getattr(abi.Keep, f).offset, f
    for f in kept_fields:
        assert got[f"kept.{f}"] == getattr(abi.Kept, f).offset == abi.KEPT_DTYPE.fields[f][1], f
    assert got["rescored_source"] == abi.ACCEPT_RESCORED == 12 and got["cohort_samples_source"] == 9
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32 and got["cohort.reserved"] == abi.Cohort.reserved.offset == 24
    assert got["select"] == C.sizeof(abi.Select) == 40 and got["accept"] == C.sizeof(abi.Accept) == 48
    assert got["accept.reserved"] == abi.Accept.reserved.offset == 40
    assert got["passages"] == C.sizeof(abi.Passages) == 24 and got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["stats"] == abi.STATS_DTYPE.itemsize == 64 and got["summary"] == abi.SUMMARY_DTYPE.itemsize == 88
    assert got["instance"] == C.sizeof(abi.Instance)
    assert got["params.subsample_cells"] == abi.Params.subsample_cells.offset
    assert got["params"] == C.sizeof(abi.Params) == PARAMS_SIZE_V13  # ecdna_ssa_params_t did not grow


def _spec(**kw):
    base = dict(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_cells=20)
    base.update(kw)
    return abi.RunSpec(**base)


def _create(lib, spec, keep, ext=None, pas=None, co=None):
    def ref(block):
        return C.byref(block) if block is not None else None

    p = spec.params()
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create_keep(C.byref(p), ref(ext), ref(pas), ref(co), ref(keep), C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_keep_rejects_bad_blocks(product_lib):
    """Before any device is touched: E_INVALID with a message that names the field, GPU or not."""
    s = _spec()
    for size in (0, C.sizeof(abi.Keep) - 4, C.sizeof(abi.Keep) + 8):
        b = s.keep()
        b.struct_size = size
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "struct_size" in msg, size
    for m in (0, 4097, (1 << 32) - 1):
        s1 = _spec(keep_cells=m)
        rc, msg = _create(product_lib, s1, s1.keep())
        assert rc == abi.E_INVALID and "keep_cells" in msg, m
    for r in (1, 1 << 40):
        b = s.keep()
        b.reserved = r
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "reserved" in msg, r
    s2 = _spec(flags=0)
    rc, msg = _create(product_lib, s2, s2.keep())
    assert rc == abi.E_INVALID and "REP_STATS" in msg
    # kept samples of every phase are a different feature: no passage block
    s3 = _spec(n_passages=2, passage_cells=5)
    rc, msg = _create(product_lib, s3, s3.keep(), pas=s3.passages())
    assert rc == abi.E_INVALID and "passages" in msg and "every phase" in msg
    # a parameter error of the params themselves, and of another block, is still reported through _keep
    s4 = _spec(hist_bins=1)
    rc, msg = _create(product_lib, s4, s4.keep())
    assert rc == abi.E_INVALID and "hist_bins" in msg
    s5 = _spec(cohort_targets=np.ones((2, BINS), dtype=np.uint64))
    co = s5.cohort()
    co.n_targets = 65
    rc, msg = _create(product_lib, s5, s5.keep(), co=co)
    assert rc == abi.E_INVALID and "n_targets" in msg


def test_create_keep_accepts_good_blocks(product_lib):
    """In range: whatever comes back (no device here, a context there), it is not a parameter error."""
    for kw in (dict(), dict(keep_cells=1), dict(keep_cells=4096), dict(keep_cells=65),
               dict(subsample_cells=7, stats_target=np.ones(BINS, dtype=np.uint64)),  # both keep their meaning
               dict(cohort_targets=np.ones((3, BINS), dtype=np.uint64), cohort_sample_cells=(20, 20, 5)),
               dict(snapshots=(2, 10), snapshot_stats=True),  # the extension block stays independent
               dict(flags=abi.FLAG_REP_STATS | abi.FLAG_BIN_STORE | abi.FLAG_EVENT_HASH, bin_kmax=32)):
        s = _spec(**kw)
        rc, msg = _create(product_lib, s, s.keep(), ext=s.ext(), co=s.cohort())
        assert rc in (abi.OK, abi.E_NODEVICE), (kw, rc, msg)
    off = _spec(keep_cells=None, flags=0)
    assert off.keep() is None  # such a spec is created without the keep entry point
    rc, msg = _create(product_lib, off, None)  # keep == NULL: ecdna_ssa_ctx_create_cohort
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    bad = abi.Cohort(struct_size=C.sizeof(abi.Cohort), n_targets=0)
    rc, msg = _create(product_lib, _spec(), None, co=bad)
    assert rc == abi.E_INVALID and "n_targets" in msg  # ... whose checks still run


def test_runspec_builds_the_block():
    b = _spec().keep()
    assert b.struct_size == C.sizeof(abi.Keep) == 16 and b.keep_cells == 20 and b.reserved == 0
    assert _spec(keep_cells=4096).keep().keep_cells == 4096
    assert abi.RunSpec().keep() is None and abi.RunSpec().keep_cells is None
    assert _spec(keep_cells=0).keep().keep_cells == 0  # (0 is a block, which the library refuses; None is no block)
    with pytest.raises(ValueError):
        _spec(keep_cells=1 << 32).keep()
    with pytest.raises(ValueError):
        _spec(keep_cells=-1).keep()
