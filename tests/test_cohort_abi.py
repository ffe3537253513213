"""A cohort of targets (ecdna_ssa_cohort_t, added within ABI v13; cohort mapping v1) without a GPU: the
header declares the block, its two entry points and the two acceptance sources, the library exports the calls, the ctypes
mirror has the header's layout, the version is still 13 and the older blocks kept their sizes, the header states the
mapping, ecdna_ssa_ctx_create_cohort validates the block before any device is touched, and RunSpec builds it."""
import ctypes as C
import re

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.abi import HEADER, PARAMS_SIZE_V13, declared, header_text, layout, product_lib  # noqa: F401 (fixture)

BINS = 9


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_create_cohort") == [
        "const ecdna_ssa_params_t* p", "const ecdna_ssa_ext_t* ext", "const ecdna_ssa_passages_t* passages",
        "const ecdna_ssa_cohort_t* cohort", "ecdna_ssa_ctx** out"]
    assert declared("ecdna_ssa_ctx_download_cohort") == [
        "ecdna_ssa_ctx* c", "ecdna_rep_stats_t* out_stats", "ecdna_rep_stats_t* out_sample_stats"]
    for name in ("ecdna_ssa_ctx_create_cohort", "ecdna_ssa_ctx_download_cohort"):
        assert hasattr(product_lib, name) and name in engine.EXPORTS
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13
    assert product_lib.ecdna_ssa_ctx_download_cohort(None, None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()


def test_the_two_sources_are_8_and_9():
    text = header_text()
    assert re.search(r"\bECDNA_ACCEPT_COHORT\s*=\s*8\s*,", text)
    assert re.search(r"\bECDNA_ACCEPT_COHORT_SAMPLES\s*=\s*9\b", text)
    assert re.search(r"\bECDNA_ACCEPT_PASSAGE_SAMPLES\s*=\s*5\s*,", text)  # the older ones did not move
    assert (abi.ACCEPT_COHORT, abi.ACCEPT_COHORT_SAMPLES) == (8, 9)
    assert (abi.ACCEPT_FINAL, abi.ACCEPT_PASSAGE_SAMPLES) == (0, 5)
    # 6 and 7 are no sources
    assert not re.search(r"\bECDNA_ACCEPT_\w+\s*=\s*[67]\b", text)


def test_the_header_states_the_cohort_mapping():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Cohort mapping v1",
                   "byte for byte the record ecdna_ssa_ctx_download_stats returns for the same run with "
                   "stats_target_hist = target_hists[p]",
                   "byte for byte the record ecdna_ssa_ctx_download_sample returns for the same run with "
                   "stats_target_hist = target_hists[p] and subsample_cells = sample_cells[p]",
                   "mean, entropy, frequency and cells are therefore the same for every p",
                   "stream field 0", "Two targets with equal sample_cells see the same sample",
                   "do not depend on chunk, shard, grid or device", "The cohort adds no pooled histograms",
                   "cohorts of longitudinal targets are a different feature",
                   "rep stride 1, timepoint stride n, error stride 0",
                   "timepoint_mask = 1 << p gives patient p's acceptance or quantiles"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): one sweep " \
           "scored against a cohort of targets" in text


def test_cohort_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror; the older blocks did not move."""
    fields = [f for f, _ in abi.Cohort._fields_]
    assert fields == ["struct_size", "n_targets", "target_hists", "sample_cells", "reserved"]
    got = layout(tmp_path, {"cohort": ("ecdna_ssa_cohort_t", fields), "select": "ecdna_ssa_select_t",
                            "accept": "ecdna_ssa_accept_t", "passages": "ecdna_ssa_passages_t", "ext": "ecdna_ssa_ext_t",
                            "stats": "ecdna_rep_stats_t", "params": "ecdna_ssa_params_t"},
                 values={"cohort_source": "ECDNA_ACCEPT_COHORT", "cohort_samples_source": "ECDNA_ACCEPT_COHORT_SAMPLES"})
    assert got["cohort"] == C.sizeof(abi.Cohort) == 32
    for f in fields:
        assert got[f"cohort.{f}"] == getattr(abi.Cohort, f).offset, f
    assert (got["cohort_source"], got["cohort_samples_source"]) == (abi.ACCEPT_COHORT, abi.ACCEPT_COHORT_SAMPLES)
    assert got["select"] == C.sizeof(abi.Select) == 40 and got["accept"] == C.sizeof(abi.Accept) == 48
    assert got["passages"] == C.sizeof(abi.Passages) == 24 and got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["stats"] == abi.STATS_DTYPE.itemsize == 64
    assert got["params"] == C.sizeof(abi.Params) == PARAMS_SIZE_V13  # ecdna_ssa_params_t did not grow


def _targets(P=3):
    return np.arange(P * BINS, dtype=np.uint64).reshape(P, BINS) + 1


def _spec(**kw):
    base = dict(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, cohort_targets=_targets(),
                cohort_sample_cells=(10, 20, 10))
    base.update(kw)
    return abi.RunSpec(**base)


def _create(lib, spec, co, ext=None, pas=None):
    p = spec.params()
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create_cohort(C.byref(p), C.byref(ext) if ext is not None else None,
                                         C.byref(pas) if pas is not None else None,
                                         C.byref(co) if co is not None else None, C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_cohort_rejects_bad_blocks(product_lib):
    """Before any device is touched: E_INVALID with a message that names the field, GPU or not."""
    s = _spec()
    for size in (0, C.sizeof(abi.Cohort) - 4, C.sizeof(abi.Cohort) + 8):
        b = s.cohort()
        b.struct_size = size
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "struct_size" in msg, size
    for P in (0, 65):
        b = s.cohort()
        b.n_targets = P
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "n_targets" in msg, P
    b = s.cohort()
    b.target_hists = C.POINTER(C.c_uint64)()
    rc, msg = _create(product_lib, s, b)
    assert rc == abi.E_INVALID and "target_hists" in msg and "NULL" in msg
    tg = _targets()
    tg[1] = 0  # an all-zero target row
    s1 = _spec(cohort_targets=tg)
    rc, msg = _create(product_lib, s1, s1.cohort())
    assert rc == abi.E_INVALID and "target_hists[1]" in msg and "empty" in msg
    for m in (0, 4097):
        s2 = _spec(cohort_sample_cells=(10, 20, m))
        rc, msg = _create(product_lib, s2, s2.cohort())
        assert rc == abi.E_INVALID and "sample_cells[2]" in msg, m
    b = s.cohort()
    b.reserved = 1
    rc, msg = _create(product_lib, s, b)
    assert rc == abi.E_INVALID and "reserved" in msg
    s3 = _spec(flags=0)
    rc, msg = _create(product_lib, s3, s3.cohort())
    assert rc == abi.E_INVALID and "REP_STATS" in msg
    # cohorts of longitudinal targets are a different feature: no passage block, no per-snapshot statistics
    s4 = _spec(n_passages=2, passage_cells=5)
    rc, msg = _create(product_lib, s4, s4.cohort(), pas=s4.passages())
    assert rc == abi.E_INVALID and "passages" in msg and "longitudinal" in msg
    s5 = _spec(snapshots=(2, 10), snapshot_stats=True)
    rc, msg = _create(product_lib, s5, s5.cohort(), ext=s5.ext())
    assert rc == abi.E_INVALID and "snapshot_stats" in msg and "longitudinal" in msg
    # a parameter error of the params themselves is still reported through _cohort
    s6 = _spec(hist_bins=1, cohort_targets=np.ones((3, 1), dtype=np.uint64))
    rc, msg = _create(product_lib, s6, s6.cohort())
    assert rc == abi.E_INVALID and "hist_bins" in msg


def test_create_cohort_accepts_good_blocks(product_lib):
    """In range: whatever comes back (no device here, a context there), it is not a parameter error."""
    for kw in (dict(), dict(cohort_sample_cells=None), dict(cohort_targets=_targets(1), cohort_sample_cells=(1,)),
               dict(cohort_targets=_targets(64), cohort_sample_cells=(4096,) * 64),
               dict(subsample_cells=7, stats_target=np.ones(BINS, dtype=np.uint64)),  # both keep their meaning
               dict(snapshots=(2, 10)),  # snapshots without their statistics are no longitudinal targets
               dict(flags=abi.FLAG_REP_STATS | abi.FLAG_BIN_STORE | abi.FLAG_EVENT_HASH, bin_kmax=32)):
        s = _spec(**kw)
        rc, msg = _create(product_lib, s, s.cohort())
        assert rc in (abi.OK, abi.E_NODEVICE), (kw, rc, msg)
    off = _spec(cohort_targets=None, cohort_sample_cells=None, flags=0)
    assert off.cohort() is None  # such a spec is created without the cohort entry point
    rc, msg = _create(product_lib, off, None)  # cohort == NULL: ecdna_ssa_ctx_create_passages
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    bad = abi.Passages(struct_size=C.sizeof(abi.Passages), n_passages=0, passage_cells=1)
    rc, msg = _create(product_lib, _spec(), None, pas=bad)
    assert rc == abi.E_INVALID and "n_passages" in msg  # ... whose checks still run


def test_runspec_builds_the_block():
    b = _spec().cohort()
    assert b.struct_size == C.sizeof(abi.Cohort) and b.n_targets == 3 and b.reserved == 0
    assert [b.target_hists[i] for i in range(3 * BINS)] == list(range(1, 3 * BINS + 1))
    assert [b.sample_cells[i] for i in range(3)] == [10, 20, 10]
    assert not _spec(cohort_sample_cells=None).cohort().sample_cells
    assert abi.RunSpec().cohort() is None
    with pytest.raises(ValueError):
        _spec(cohort_targets=np.ones((3, BINS + 1), dtype=np.uint64)).cohort()  # hist_bins entries per target
    with pytest.raises(ValueError):
        _spec(cohort_sample_cells=(10, 20)).cohort()  # one sample size per target
    with pytest.raises(ValueError):
        _spec(cohort_sample_cells=(10, 20, 1 << 32)).cohort()
    with pytest.raises(ValueError):
        _spec(cohort_targets=None).cohort()  # sample sizes without targets
