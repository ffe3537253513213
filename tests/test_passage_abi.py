"""Serial passaging (ecdna_ssa_passages_t, added within ABI v13) without a GPU: the header declares the
passage block and its two entry points, the library exports them, the ctypes mirror has the header's layout, the version
is still 13 and the older blocks kept their sizes, and ecdna_ssa_ctx_create_passages validates the block before any
device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.abi import PARAMS_SIZE_V13, declared, header_text, layout, product_lib  # noqa: F401 (fixture)


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_create_passages") == [
        "const ecdna_ssa_params_t* p", "const ecdna_ssa_ext_t* ext", "const ecdna_ssa_passages_t* passages",
        "ecdna_ssa_ctx** out"]
    assert declared("ecdna_ssa_ctx_download_passages") == [
        "ecdna_ssa_ctx* c", "ecdna_rep_summary_t* out_summaries", "ecdna_totals_t* out_totals",
        "ecdna_rep_stats_t* out_stats", "ecdna_rep_stats_t* out_sample_stats", "uint64_t* out_hist",
        "uint64_t* out_sample_hist"]
    for name in ("ecdna_ssa_ctx_create_passages", "ecdna_ssa_ctx_download_passages"):
        assert hasattr(product_lib, name) and name in engine.EXPORTS
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13
    assert product_lib.ecdna_ssa_ctx_download_passages(None, None, None, None, None, None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()


def test_passages_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror; the older blocks did not move."""
    fields = [f for f, _ in abi.Passages._fields_]
    assert fields == ["struct_size", "n_passages", "passage_cells", "reserved", "passage_target_hists"]
    got = layout(tmp_path, {"passages": ("ecdna_ssa_passages_t", fields), "ext": "ecdna_ssa_ext_t",
                            "params": "ecdna_ssa_params_t"})
    assert got["passages"] == C.sizeof(abi.Passages) == 24
    for f in fields:
        assert got[f"passages.{f}"] == getattr(abi.Passages, f).offset, f
    assert got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["params"] == C.sizeof(abi.Params) == PARAMS_SIZE_V13  # ecdna_ssa_params_t did not grow


def _spec(**kw):
    base = dict(n_replicates=4, max_cells=50, hist_bins=9, flags=abi.FLAG_REP_STATS, n_passages=3, passage_cells=10)
    base.update(kw)
    return abi.RunSpec(**base)


def _create(lib, spec, pas, ext=None):
    p = spec.params()
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create_passages(C.byref(p), C.byref(ext) if ext is not None else None,
                                           C.byref(pas) if pas is not None else None, C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_passages_rejects_bad_blocks(product_lib):
    """Before any device is touched: E_INVALID with a message that names the field, GPU or not."""
    s = _spec()
    b = s.passages()
    assert b.struct_size == C.sizeof(abi.Passages) and b.n_passages == 3 and b.passage_cells == 10
    assert not b.passage_target_hists and b.reserved == 0
    for size in (0, C.sizeof(abi.Passages) - 4, C.sizeof(abi.Passages) + 8):
        b = s.passages()
        b.struct_size = size
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "struct_size" in msg, size
    b = s.passages()
    b.reserved = 1
    rc, msg = _create(product_lib, s, b)
    assert rc == abi.E_INVALID and "reserved" in msg
    for g in (0, 17):
        b = s.passages()
        b.n_passages = g
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "n_passages" in msg, g
    for m in (0, 4097):
        b = s.passages()
        b.passage_cells = m
        rc, msg = _create(product_lib, s, b)
        assert rc == abi.E_INVALID and "passage_cells" in msg, m
    s1 = _spec(passage_cells=51, cell_cap=50)  # a sample the rows could not hold
    rc, msg = _create(product_lib, s1, s1.passages())
    assert rc == abi.E_INVALID and "passage_cells" in msg and "cell_cap" in msg
    s2 = _spec(flags=0)
    rc, msg = _create(product_lib, s2, s2.passages())
    assert rc == abi.E_INVALID and "REP_STATS" in msg
    s3 = _spec(subsample_cells=5)  # the block owns the sample size
    rc, msg = _create(product_lib, s3, s3.passages())
    assert rc == abi.E_INVALID and "subsample_cells" in msg
    s4 = _spec(snapshots=(2, 10))
    rc, msg = _create(product_lib, s4, s4.passages())
    assert rc == abi.E_INVALID and "n_snapshots" in msg
    s5 = _spec(snapshots=(2, 10), snapshot_stats=True)
    rc, msg = _create(product_lib, s5, s5.passages(), s5.ext())
    assert rc == abi.E_INVALID and ("n_snapshots" in msg or "snapshot_stats" in msg)
    e = abi.Ext(struct_size=C.sizeof(abi.Ext), snapshot_stats=1)  # snapshot_stats without snapshots: the ext's own check
    rc, msg = _create(product_lib, s, s.passages(), e)
    assert rc == abi.E_INVALID and ("snapshot_stats" in msg or "n_snapshots" in msg)
    s6 = _spec(flags=abi.FLAG_REP_STATS | abi.FLAG_REFERENCE_DRAWS)
    rc, msg = _create(product_lib, s6, s6.passages())
    assert rc == abi.E_INVALID and "REFERENCE_DRAWS" in msg
    tg = np.ones((3, 9), dtype=np.uint64)
    tg[2] = 0  # an all-zero target row
    s7 = _spec(passage_targets=tg)
    rc, msg = _create(product_lib, s7, s7.passages())
    assert rc == abi.E_INVALID and "passage_target_hists[2]" in msg and "empty" in msg
    # a parameter error of the params themselves is still reported through _passages
    s8 = _spec(hist_bins=1)
    rc, msg = _create(product_lib, s8, s8.passages())
    assert rc == abi.E_INVALID and "hist_bins" in msg


def test_create_passages_accepts_good_blocks(product_lib):
    """In range: whatever comes back (no device here, a context there), it is not a parameter error."""
    tg = np.ones((3, 9), dtype=np.uint64)
    for kw in (dict(), dict(passage_targets=tg), dict(n_passages=1, passage_cells=1),
               dict(n_passages=16, passage_cells=4096, max_cells=5000),
               dict(flags=abi.FLAG_REP_STATS | abi.FLAG_BIN_STORE | abi.FLAG_EVENT_HASH, bin_kmax=32, big_cap=2),
               dict(stats_target=np.ones(9, dtype=np.uint64))):
        s = _spec(**kw)
        rc, msg = _create(product_lib, s, s.passages())
        assert rc in (abi.OK, abi.E_NODEVICE), (kw, rc, msg)
    off = _spec(n_passages=0, passage_cells=0, flags=0)
    assert off.passages() is None  # such a spec is created without the passage entry point
    rc, msg = _create(product_lib, off, None)  # passages == NULL: ecdna_ssa_ctx_create_ext
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    rc, msg = _create(product_lib, off, None, abi.Ext(struct_size=C.sizeof(abi.Ext), reserved=3))
    assert rc == abi.E_INVALID and "reserved" in msg  # ... whose checks still run


def test_runspec_builds_the_block():
    tg = np.arange(27, dtype=np.uint64).reshape(3, 9) + 1
    b = _spec(passage_targets=tg).passages()
    assert [b.passage_target_hists[i] for i in range(27)] == list(range(1, 28))
    with pytest.raises(ValueError):
        _spec(passage_targets=np.ones((2, 9), dtype=np.uint64)).passages()  # one histogram per passage
    with pytest.raises(ValueError):
        _spec(passage_cells=1 << 32).passages()
    assert abi.RunSpec().passages() is None
