"""Per-snapshot ABC statistics (ecdna_ssa_ext_t, added within ABI v13) without a GPU: the header
declares the extension block and its two entry points, the library exports them, the ctypes mirror has the header's
layout, the version is still 13, and ecdna_ssa_ctx_create_ext validates the block before any device is touched. The
numpy restatement the GPU tests compare against (tests/snapshot_stats_law.py) differs from the end-of-run sample's in
the stream field only."""
import ctypes as C
import re

import numpy as np
import pytest

import snapshot_stats_law as ssl
import subsample_law as sl
from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_create_ext") == [
        "const ecdna_ssa_params_t* p", "const ecdna_ssa_ext_t* ext", "ecdna_ssa_ctx** out"]
    assert declared("ecdna_ssa_ctx_download_snapshot_stats") == [
        "ecdna_ssa_ctx* c", "ecdna_rep_stats_t* out_stats", "ecdna_rep_stats_t* out_sample_stats", "uint64_t* out_hist",
        "uint64_t* out_sample_hist"]
    for name in ("ecdna_ssa_ctx_create_ext", "ecdna_ssa_ctx_download_snapshot_stats"):
        assert hasattr(product_lib, name) and name in engine.EXPORTS
    # additive: the version, and the tail of the parameter block, are v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13
    assert [f for f, _ in abi.Params._fields_][-3:] == ["reserved0", "subsample_cells", "reserved1"]
    assert "within v13" in open(HEADER).read()
    assert product_lib.ecdna_ssa_ctx_download_snapshot_stats(None, None, None, None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()


def test_ext_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror (as tests/test_abi.py)."""
    fields = [f for f, _ in abi.Ext._fields_]
    assert fields == ["struct_size", "snapshot_stats", "snapshot_target_hists", "snapshot_subsample_cells", "reserved"]
    got = layout(tmp_path, {"ext": ("ecdna_ssa_ext_t", fields), "params": "ecdna_ssa_params_t"})
    assert got["ext"] == C.sizeof(abi.Ext) == 24
    for f in fields:
        assert got[f"ext.{f}"] == getattr(abi.Ext, f).offset, f
    assert got["params"] == C.sizeof(abi.Params)  # ecdna_ssa_params_t did not grow


def _spec(**kw):
    base = dict(n_replicates=4, max_cells=50, hist_bins=9, flags=abi.FLAG_REP_STATS, snapshots=(2, 10),
                snapshot_stats=True)
    base.update(kw)
    return abi.RunSpec(**base)


def _create_ext(lib, spec, ext):
    p = spec.params()
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create_ext(C.byref(p), C.byref(ext) if ext is not None else None, C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_ext_rejects_bad_blocks(product_lib):
    """Before any device is touched: E_INVALID with a message that names the field, GPU or not."""
    s = _spec()
    e = s.ext()
    assert e.struct_size == C.sizeof(abi.Ext) and e.snapshot_stats == 1 and not e.snapshot_target_hists
    e.struct_size = C.sizeof(abi.Ext) - 4
    rc, msg = _create_ext(product_lib, s, e)
    assert rc == abi.E_INVALID and "struct_size" in msg
    e = s.ext()
    e.struct_size = 0
    rc, msg = _create_ext(product_lib, s, e)
    assert rc == abi.E_INVALID and "struct_size" in msg
    e = s.ext()
    e.reserved = 1
    rc, msg = _create_ext(product_lib, s, e)
    assert rc == abi.E_INVALID and "reserved" in msg
    s2 = _spec(snapshots=None)  # no snapshots
    rc, msg = _create_ext(product_lib, s2, s2.ext())
    assert rc == abi.E_INVALID and "n_snapshots" in msg
    s3 = _spec(flags=0)  # no ECDNA_FLAG_REP_STATS
    rc, msg = _create_ext(product_lib, s3, s3.ext())
    assert rc == abi.E_INVALID and "REP_STATS" in msg
    tg = np.ones((2, 9), dtype=np.uint64)
    tg[1] = 0  # an all-zero target
    s4 = _spec(snapshot_targets=tg)
    rc, msg = _create_ext(product_lib, s4, s4.ext())
    assert rc == abi.E_INVALID and "snapshot_target_hists[1]" in msg and "empty" in msg
    s5 = _spec(snapshot_subsample_cells=4097)
    rc, msg = _create_ext(product_lib, s5, s5.ext())
    assert rc == abi.E_INVALID and "snapshot_subsample_cells" in msg and "4096" in msg
    # the block is checked even when the feature is off
    e = abi.Ext(struct_size=C.sizeof(abi.Ext), reserved=7)
    rc, msg = _create_ext(product_lib, _spec(snapshot_stats=False), e)
    assert rc == abi.E_INVALID and "reserved" in msg
    # a parameter error of the params themselves is still reported through _ext
    p_bad = _spec(subsample_cells=4097)
    rc, msg = _create_ext(product_lib, p_bad, p_bad.ext())
    assert rc == abi.E_INVALID and "subsample_cells" in msg


def test_create_ext_accepts_good_blocks(product_lib):
    """In range: whatever comes back (no device here, a context there), it is not a parameter error."""
    tg = np.ones((2, 9), dtype=np.uint64)
    for kw in (dict(), dict(snapshot_targets=tg), dict(snapshot_subsample_cells=1), dict(snapshot_subsample_cells=4096),
               dict(snapshot_targets=tg, snapshot_subsample_cells=100, flags=abi.FLAG_REP_STATS | abi.FLAG_SNAPSHOT_ROWS)):
        s = _spec(**kw)
        rc, msg = _create_ext(product_lib, s, s.ext())
        assert rc in (abi.OK, abi.E_NODEVICE), (kw, rc, msg)
    off = _spec(snapshot_stats=False, snapshots=None, flags=0)
    assert off.ext() is None  # such a spec is created by ecdna_ssa_ctx_create
    for ext in (None, abi.Ext(struct_size=C.sizeof(abi.Ext))):  # ext == NULL, and snapshot_stats == 0
        rc, msg = _create_ext(product_lib, off, ext)
        assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)


def test_runspec_builds_the_block():
    tg = np.arange(18, dtype=np.uint64).reshape(2, 9) + 1
    s = _spec(snapshot_targets=tg, snapshot_subsample_cells=77)
    e = s.ext()
    assert e.snapshot_subsample_cells == 77 and e.reserved == 0
    assert [e.snapshot_target_hists[i] for i in range(18)] == list(range(1, 19))
    with pytest.raises(ValueError):
        _spec(snapshot_targets=np.ones((3, 9), dtype=np.uint64)).ext()  # one histogram per snapshot
    with pytest.raises(ValueError):
        _spec(snapshot_subsample_cells=1 << 32).ext()
    assert abi.RunSpec().ext() is None


def test_the_snapshot_stream_differs_from_the_end_of_run_stream_in_the_field_only():
    """With the field (s + 1) << 16 forced to 0 the restatement draws the end-of-run sample exactly; with s = 0 (field
    0x10000) it does not, nor do two snapshots draw the same sample."""
    assert ssl.stream_field(0) == 0x10000 and ssl.stream_field(63) == 0x400000
    assert all(ssl.stream_field(s) & 0x3FF == 0 and ssl.stream_field(s) < sl.TAG for s in range(64))  # clear of t
    for N, m in ((40, 10), (2000, 700), (2000, 1500), (2000, 1999), (65, 64), (8200, 4096)):
        for rid in (0, 5, 2**40 + 3):
            want, want_comp = sl.sample_positions(N, m, 9, rid)
            got, comp = ssl.sample_positions(N, m, 9, rid, 0, field=0)
            assert comp == want_comp and np.array_equal(got, want), (N, m, rid)
            s0, comp0 = ssl.sample_positions(N, m, 9, rid, 0)
            assert comp0 == want_comp and len(s0) == len(want) == len(np.unique(s0)) and s0.max() < N
            if min(m, N - m) >= 10:  # (a pick of a few positions can coincide by chance)
                assert not np.array_equal(s0, want), (N, m, rid)
                assert not np.array_equal(s0, ssl.sample_positions(N, m, 9, rid, 1)[0])
    np.testing.assert_array_equal(ssl.draws(3, 50, 1000, 7, 11, 0), sl.draws(3, 50, 1000, 7, 11))
    for N, m in ((0, 5), (5, 5), (5, 9)):  # m >= N: everything, in order
        pos, comp = ssl.sample_positions(N, m, 1, 2, 3)
        assert pos.tolist() == list(range(N)) and not comp


def test_restatement_of_a_snapshot():
    """Not taken: the empty population (ks 1.0 with a target); taken: the statistics of n- and the row's first n+."""
    import abc_stats

    bins = 17
    tg = np.zeros(bins, np.uint64)
    tg[:6] = 4
    meta = np.zeros(2, dtype=abi.SNAPSHOT_DTYPE)
    meta[1] = (0.5, 7, 5, 1, 0)
    row = np.asarray([1, 2, 40, 3, 3, 9, 9, 9], dtype=np.uint16)  # entries past n+ are not part of the state
    st, h = ssl.full(meta[0], row, bins, tg)
    assert st["cells"] == 0 and st["ks"] == 1.0 and st["mean"] == 0.0 and not h.any()
    assert ssl.sample(meta[0], row, 3, 1, 2, 0, bins, tg)[0] == st
    st, h = ssl.full(meta[1], row, bins, tg)
    assert st == abc_stats.rep_stats(7, row[:5], bins, tg) and int(h[0]) == 7 and int(h[16]) == 1 and int(h.sum()) == 12
    assert ssl.sample(meta[1], row, 12, 1, 2, 0, bins, tg)[0] == st  # m = N: the whole state
    for m in (1, 5, 8, 11):
        sst, sh = ssl.sample(meta[1], row, m, 1, 2, 0, bins, tg)
        assert sst["cells"] == m == int(sh.sum()) and np.all(sh <= h)


def test_gather_structured_takes_per_snapshot_records(tmp_path):
    """shard.gather_structured moves [n][S] records as raw bytes and still returns [n] for one record per replicate
    (a one-rank gloo group in this process)."""
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    rng = np.random.default_rng(1)
    two = np.frombuffer(rng.bytes(7 * 3 * abi.STATS_DTYPE.itemsize), dtype=abi.STATS_DTYPE).reshape(7, 3)
    one = np.frombuffer(rng.bytes(7 * abi.STATS_DTYPE.itemsize), dtype=abi.STATS_DTYPE)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        got2 = shard.gather_structured(two, 7, "interleaved")
        got1 = shard.gather_structured(one, 7, "contiguous")
    finally:
        dist.destroy_process_group()
    assert got2.dtype == abi.STATS_DTYPE and got2.shape == (7, 3) and got2.tobytes() == two.tobytes()
    assert got1.shape == (7,) and got1.tobytes() == one.tobytes()
