"""Per-snapshot ABC statistics on the GPU (ecdna_ssa_ext_t, added within ABI v13). Snapshot states come
from engine.run and are first checked against the oracle (metadata, sorted rows), so the statistics are judged on states
the oracle vouches for; the statistics, the samples' statistics and the histograms are compared with the numpy
restatement (tests/snapshot_stats_law.py) applied to the run's own snapshot rows: integers exactly, floats at the
ABC-statistics tolerance of tests/test_gpu_abc_stats.py (1e-12 relative: sums are reduced in a different order on the
GPU; log is ocml's vs numpy's). One test checks the sample's law independently of the restatement."""
import ctypes as C

import numpy as np
import pytest

import snapshot_stats_law as ssl
from ecdna_evo_amd import abi
from exact_law import chi2_lumped
from support.snapshot_specs import BINS, SNAPS, _spec, _store_flags

RTOL, ATOL = 1e-12, 1e-14
FLOATS = ("mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")
# rows, the bin store at every K (the 300-copy cell lies in the large-k row of each), and the reference draws
STORES = [("rows", 0), ("bins", 32), ("bins", 64), ("bins", 256), ("refdraws", 0)]
# (999: the complement with m' = 1 at the 1000-cell snapshot, beside the sizes the ABC tests use)
SAMPLE_SIZES = (1, 63, 64, 65, 700, 999, 1500, 1999, 2000, 4096)
_ORACLE = {}
_FULL = {}


def dataclass_replace(spec, **kw):
    import dataclasses

    return dataclasses.replace(spec, _keep=[], _keep_ext=[], **kw)


def _oracle(oracle_mod, store, kmax, spec):
    """One oracle run per store (neither the targets nor the sample size change the states), shared, left unchanged."""
    key = (store, kmax)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run(spec, mode="compat" if store == "refdraws" else "philox")
    return _ORACLE[key]


def _check_states(g, c, spec):
    """The snapshot metadata and the sorted snapshot rows are the oracle's."""
    np.testing.assert_array_equal(g.summaries["event_hash"], c.summaries["event_hash"])
    for f in ("nminus", "nplus", "taken"):
        np.testing.assert_array_equal(g.snapshots[f], c.snapshots[f], err_msg=f)
    np.testing.assert_array_equal(g.snapshots["time"].view(np.uint64), c.snapshots["time"].view(np.uint64))
    for i in range(spec.n_replicates):
        for s in range(len(spec.snapshots)):
            np.testing.assert_array_equal(np.sort(g.snapshot_row(i, s)), np.sort(c.snapshot_row(i, s)),
                                          err_msg=f"snapshot row {i}/{s}")


def _compare(got, want, what):
    """got: [n][S] abi.STATS_DTYPE; want: [n][S] restated (statistics, histogram) pairs."""
    cells = np.asarray([[w[0]["cells"] for w in r] for r in want], dtype=np.uint64)
    np.testing.assert_array_equal(got["cells"], cells, err_msg=f"{what}: cells")
    for f in FLOATS:
        np.testing.assert_allclose(got[f], np.asarray([[w[0][f] for w in r] for r in want]), rtol=RTOL, atol=ATOL,
                                   err_msg=f"{what}: {f}")


def _sum_hists(want, spec):
    """[S][sets][bins]: per snapshot and set, the sum of the restated histograms."""
    rps = spec.reps_per_set or spec.last_replicate() + 1
    out = np.zeros((len(spec.snapshots), len(spec.rates), spec.hist_bins), dtype=np.uint64)
    for i, rid in enumerate(spec.replicate_ids()):
        for s in range(len(spec.snapshots)):
            out[s, int(rid) // rps] += want[i][s][1]
    return out


def _check_full(g, spec, key=None):
    """snapshot_stats and snapshot_hist against the restatement applied to the run's own snapshot rows. `key`: the
    restatement of these states is shared under it (the sample size does not change it) and left unchanged."""
    S, bins, tg = len(spec.snapshots), spec.hist_bins, spec.snapshot_targets
    assert g.snapshot_stats.dtype == abi.STATS_DTYPE and g.snapshot_stats.shape == (spec.n_replicates, S)
    assert g.snapshot_hist.dtype == np.uint64 and g.snapshot_hist.shape == (S, len(spec.rates), bins)
    if key is None or key not in _FULL:
        want = [[ssl.full(g.snapshots[i, s], g.snapshot_rows[i, s], bins, None if tg is None else tg[s])
                 for s in range(S)] for i in range(spec.n_replicates)]
        if key is not None:
            _FULL[key] = want
    else:
        want = _FULL[key]
    _compare(g.snapshot_stats, want, "snapshot_stats")
    np.testing.assert_array_equal(g.snapshot_hist, _sum_hists(want, spec))
    taken = g.snapshots["taken"] == 1
    assert taken.any() and (~taken).any()  # the run has taken snapshots and snapshots that were not
    assert taken[:, 0].all() and not taken[:, -1].any() and 0 < (~taken[:, 1]).sum() < 30  # (extinct before 40 cells)
    assert np.all(g.snapshot_stats["cells"][~taken] == 0)
    assert np.all(g.snapshot_stats["cells"][taken] == np.broadcast_to(np.asarray(spec.snapshots), taken.shape)[taken])
    for f in ("mean", "entropy", "frequency"):
        assert np.all(g.snapshot_stats[f][~taken] == 0.0)
    assert np.all(g.snapshot_stats["ks"][~taken] == (1.0 if tg is not None else 0.0))


def _check_samples(g, spec, tag=""):
    S, bins, tg, m = len(spec.snapshots), spec.hist_bins, spec.snapshot_targets, spec.snapshot_subsample_cells
    ids = spec.replicate_ids()
    assert g.snapshot_sample_stats.dtype == abi.STATS_DTYPE and g.snapshot_sample_stats.shape == (spec.n_replicates, S)
    assert g.snapshot_sample_hist.shape == (S, len(spec.rates), bins)
    want = [[ssl.sample(g.snapshots[i, s], g.snapshot_rows[i, s], m, spec.seed, int(ids[i]), s, bins,
                        None if tg is None else tg[s]) for s in range(S)] for i in range(spec.n_replicates)]
    _compare(g.snapshot_sample_stats, want, f"{tag} snapshot_sample_stats")
    np.testing.assert_array_equal(g.snapshot_sample_stats["cells"], np.minimum(g.snapshot_stats["cells"], m))
    np.testing.assert_array_equal(g.snapshot_sample_hist, _sum_hists(want, spec), err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
@pytest.mark.parametrize("with_target", [False, True])
def test_snapshot_stats_match_restatement(engine_mod, oracle_mod, with_target, store, kmax):
    spec = _spec(store, kmax, with_target, 0)
    g = engine_mod.run(spec)
    _check_states(g, _oracle(oracle_mod, store, kmax, spec), spec)
    assert g.snapshot_sample_stats is None and g.snapshot_sample_hist is None
    _check_full(g, spec)
    if with_target:  # each snapshot against its own target: the same state scores differently against another's
        tg = spec.snapshot_targets
        i = int(np.flatnonzero(g.snapshots["taken"][:, 3] == 1)[0])
        other = ssl.full(g.snapshots[i, 3], g.snapshot_rows[i, 3], BINS, tg[2])[0]
        assert abs(other["ks"] - float(g.snapshot_stats[i, 3]["ks"])) > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("m", SAMPLE_SIZES)
@pytest.mark.parametrize("store,kmax", STORES)
@pytest.mark.parametrize("with_target", [False, True])
def test_snapshot_sample_stats_match_restatement(engine_mod, oracle_mod, with_target, store, kmax, m):
    """Sample sizes at, before and after a 64-draw batch edge (63, 64, 65), through the complement (700 of 1000; 1500
    and 1999 of 2000 do not occur: the snapshot at 2000 cells is never taken, so 700 is the complement's case, m' = 300)
    and the whole population (every m >= the snapshot's cells; 2000 and 4096 for every snapshot)."""
    spec = _spec(store, kmax, with_target, m)
    g = engine_mod.run(spec)
    _check_states(g, _oracle(oracle_mod, store, kmax, spec), spec)
    _check_full(g, spec, key=(store, kmax, with_target))
    _check_samples(g, spec, f"m = {m}")
    if m >= 2000:  # every sample is its population: the full snapshot statistics, field for field
        for f in FLOATS + ("cells",):
            np.testing.assert_array_equal(g.snapshot_sample_stats[f], g.snapshot_stats[f], err_msg=f)
        np.testing.assert_array_equal(g.snapshot_sample_hist, g.snapshot_hist)
    else:
        taken = g.snapshots["taken"] == 1
        cells = g.snapshot_stats["cells"]
        assert np.all(g.snapshot_sample_stats["cells"][taken] == np.minimum(cells[taken], m))
        assert np.all(g.snapshot_sample_stats["cells"][~taken] == 0)
        if with_target:
            assert np.all(g.snapshot_sample_stats["ks"][~taken] == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_limits(engine_mod, oracle_mod, store, kmax):
    """The largest table (m' = 4096 of 8,200 cells) beside the largest histogram (2,048 bins): one wave per workgroup,
    and no room in LDS for the workgroup's sum of the samples' histograms, which the waves then add to global memory."""
    spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8300, hist_bins=2048,
                       flags=abi.FLAG_REP_STATS | abi.FLAG_SNAPSHOT_ROWS | abi.FLAG_EVENT_HASH | _store_flags(store),
                       bin_kmax=kmax, snapshots=(5000, 8200), snapshot_stats=True, snapshot_subsample_cells=4096)
    g = engine_mod.run(spec)
    _check_states(g, oracle_mod.run(spec), spec)
    assert np.all(g.snapshots["taken"] == 1) and np.all(g.snapshot_stats["cells"] == (5000, 8200))
    want = [[ssl.full(g.snapshots[i, s], g.snapshot_rows[i, s], 2048) for s in range(2)] for i in range(64)]
    _compare(g.snapshot_stats, want, "snapshot_stats")
    np.testing.assert_array_equal(g.snapshot_hist, _sum_hists(want, spec))
    _check_samples(g, spec)  # 5000 cells: the complement (m' = 904); 8200: m' = m = 4096
    assert np.all(g.snapshot_sample_stats["cells"] == 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
def test_last_snapshot_is_the_final_state(engine_mod, store, kmax):
    """Replicates that stopped at max_cells = 2000 with the last snapshot taken: their last-snapshot statistics are
    result.stats bit for bit. In this spec the selection is EMPTY for every store — a replicate that reaches max_cells
    stops before the snapshot rule runs (the stop checks come first), so the snapshot at max_cells is
    never taken. The same comparison is therefore made where it can bind: the run again with max_cells = 4000 and the
    same time limit draws the same events up to its first 2000 cells, where it takes the snapshot the first run
    stopped at."""
    spec = _spec(store, kmax, True, 0, max_time=14.0)
    tg = spec.snapshot_targets
    g = engine_mod.run(dataclass_replace(spec, stats_target=tg[-1]))
    sel = (g.summaries["stop_reason"] == abi.STOP_MAX_CELLS) & (g.snapshots["taken"][:, -1] == 1)
    print(f"{store} K={kmax}: stopped at max_cells with the last snapshot taken: {int(sel.sum())}")
    assert g.snapshot_stats[sel, -1].tobytes() == g.stats[sel].tobytes()
    longer = engine_mod.run(dataclass_replace(spec, stats_target=tg[-1], max_cells=4000))
    sel = (g.summaries["stop_reason"] == abi.STOP_MAX_CELLS) & (longer.snapshots["taken"][:, -1] == 1)
    assert sel.sum() >= 590 and np.array_equal(sel, g.summaries["stop_reason"] == abi.STOP_MAX_CELLS)
    for f in ("nminus", "nplus"):
        np.testing.assert_array_equal(longer.snapshots[f][sel, -1], g.summaries[f][sel])
    assert longer.snapshot_stats[sel, -1].tobytes() == g.stats[sel].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_layout_independence(engine_mod, store, kmax, monkeypatch):
    """Without FLAG_SNAPSHOT_ROWS the snapshot rows are one chunk's scratch: seven uneven chunks that straddle the set
    boundary, and two interleaved shards, give the one-chunk run's per-replicate arrays exactly; the shards' histograms
    sum to its."""
    whole = engine_mod.run(_spec(store, kmax, True, 700))
    assert whole.snapshot_rows is not None
    per_rep = ("snapshot_stats", "snapshot_sample_stats", "stats", "summaries", "snapshots")
    hists = ("snapshot_hist", "snapshot_sample_hist", "hist")
    total = {h: np.zeros_like(getattr(whole, h)) for h in hists}
    for gi in range(2):
        part = engine_mod.run(_spec(store, kmax, True, 700, flags=abi.FLAG_EVENT_HASH, first_replicate=gi,
                                    replicate_stride=2, n_replicates=300))
        assert part.snapshot_rows is None
        for f in per_rep:
            assert getattr(part, f).tobytes() == getattr(whole, f)[gi::2].tobytes(), f"shard {gi}: {f}"
        for h in hists:
            total[h] += getattr(part, h)
    for h in hists:
        np.testing.assert_array_equal(total[h], getattr(whole, h), err_msg=h)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "97")
    with engine_mod.Context(_spec(store, kmax, True, 700, flags=abi.FLAG_EVENT_HASH)) as ctx:
        assert ctx.instance()["n_chunks"] == 7
        ctx.launch()
        ctx.sync()
        chunked = ctx.download()
        rows = np.zeros((600, len(SNAPS), 2048), dtype=np.uint16)
        rc = engine_mod.lib().ecdna_ssa_ctx_download_snapshots(ctx.h, None, rows.ctypes.data)
        assert rc == abi.E_STATE and b"SNAPSHOT_ROWS" in engine_mod.lib().ecdna_ssa_last_error_message()
    assert chunked.snapshot_rows is None
    for f in per_rep:
        assert getattr(chunked, f).tobytes() == getattr(whole, f).tobytes(), f
    for h in hists:
        np.testing.assert_array_equal(getattr(chunked, h), getattr(whole, h), err_msg=h)
    # with the rows kept for the whole run, a chunked run still hands them out, and computes the same
    with engine_mod.Context(_spec(store, kmax, True, 700)) as ctx:
        assert ctx.instance()["n_chunks"] == 7
        ctx.launch()
        ctx.sync()
        kept = ctx.download()
    assert kept.snapshot_rows.tobytes() == whole.snapshot_rows.tobytes()
    for f in per_rep:
        assert getattr(kept, f).tobytes() == getattr(whole, f).tobytes(), f


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_snapshot_sample_law_is_hypergeometric(engine_mod, store, kmax):
    """Independent of the restatement: 25 N- and 15 N+ cells, saved by the snapshot at 40 cells before the first event,
    sampled 10 at a time: the N+ cells in the sample are Hypergeometric(40, 15, 10). The same statistic and threshold
    as tests/test_gpu_subsample_stats.py's."""
    from scipy import stats

    n = 65536
    spec = abi.RunSpec(seed=2025, process=abi.PURE_BIRTH, n_replicates=n, max_cells=41, hist_bins=17,
                       init={0: 25, 1: 15}, flags=abi.FLAG_REP_STATS | _store_flags(store), bin_kmax=kmax,
                       snapshots=(40,), snapshot_stats=True, snapshot_subsample_cells=10)
    g = engine_mod.run(spec)
    assert np.all(g.snapshots["taken"] == 1) and np.all(g.snapshots["nplus"] == 15) and np.all(g.snapshots["time"] == 0)
    assert np.all(g.summaries["iters"] == 1) and g.snapshot_rows is None
    assert np.all(g.snapshot_stats["cells"] == 40) and np.all(g.snapshot_sample_stats["cells"] == 10)
    freq = g.snapshot_sample_stats["frequency"][:, 0]
    x = np.rint(freq * 10).astype(np.int64)  # N+ cells of the sample: cells - hist[0]
    np.testing.assert_allclose(freq * 10, x, rtol=0, atol=1e-9)
    np.testing.assert_allclose(g.snapshot_sample_stats["mean"][:, 0] * 10, x, rtol=0, atol=1e-9)  # one copy each
    obs = np.bincount(x, minlength=11)
    assert len(obs) == 11
    assert int(g.snapshot_sample_hist[0, 0, 1]) == int(x.sum())
    assert int(g.snapshot_sample_hist[0, 0, 0]) == 10 * n - int(x.sum())
    assert int(g.snapshot_hist[0, 0, 0]) == 25 * n and int(g.snapshot_hist[0, 0, 1]) == 15 * n
    p = chi2_lumped(obs, stats.hypergeom.pmf(np.arange(11), 40, 15, 10) * n, min_expected=5)
    assert p > 1e-6, (p, obs.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_feature_off_changes_nothing(engine_mod, store, kmax):
    """Through ecdna_ssa_ctx_create_ext with snapshot_stats = 0, and through ecdna_ssa_ctx_create, every output is the
    same, and there are no snapshot statistics to download; on, nothing else moves."""
    L = engine_mod.lib()
    off_spec = _spec(store, kmax, False, 0, snapshot_stats=False, subsample_cells=200)
    assert off_spec.ext() is None
    outs = []
    for ext in (None, abi.Ext(struct_size=C.sizeof(abi.Ext), snapshot_stats=0, snapshot_subsample_cells=300)):
        with engine_mod.Context(off_spec, ext=ext) as ctx:
            assert L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, None, None, None, None) == abi.E_STATE
            ctx.launch()
            ctx.sync()
            outs.append(ctx.download(want_rows=True))
            st = np.zeros((600, len(SNAPS)), dtype=abi.STATS_DTYPE)
            rc = L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, st.ctypes.data, None, None, None)
            assert rc == abi.E_STATE and L.ecdna_ssa_last_error_message() and not st.view(np.uint8).any()
    on_spec = _spec(store, kmax, True, 0, subsample_cells=200)
    with engine_mod.Context(on_spec) as ctx:
        assert L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, None, None, None, None) == abi.E_STATE  # before a launch
        ctx.launch()
        ctx.sync()
        outs.append(ctx.download(want_rows=True))
        assert L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, None, None, None, None) == abi.OK  # all may be NULL
        st = np.zeros((600, len(SNAPS)), dtype=abi.STATS_DTYPE)
        rc = L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, None, st.ctypes.data, None, None)
        assert rc == abi.E_STATE  # a sample buffer with snapshot_subsample_cells == 0
        sh = np.zeros((len(SNAPS), 2, BINS), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_download_snapshot_stats(ctx.h, None, None, None, sh.ctypes.data) == abi.E_STATE
    a, b, on = outs
    for r in (a, b):
        assert r.snapshot_stats is None and r.snapshot_hist is None and r.snapshot_sample_stats is None
    assert on.snapshot_stats is not None and on.snapshot_sample_stats is None
    for other in (b, on):
        for f in ("summaries", "totals", "stats", "hist", "sample_stats", "sample_hist", "snapshots"):
            assert getattr(a, f).tobytes() == getattr(other, f).tobytes(), f
        for i in range(600):
            np.testing.assert_array_equal(a.row(i), other.row(i))
            for s in range(len(SNAPS)):
                np.testing.assert_array_equal(a.snapshot_row(i, s), other.snapshot_row(i, s))


@pytest.mark.gpu
def test_gather_structured_takes_snapshot_stats(engine_mod, tmp_path):
    """shard.gather_structured moves the [n][S] statistics as raw bytes, as it moves the end-of-run statistics (a
    one-rank gloo group in this process; tests/test_gpu_abc_gather.py runs the exchange across ranks)."""
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    res = engine_mod.run(_spec("bins", 64, True, 128))
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        got = [shard.gather_structured(a, 600, "interleaved") for a in (res.snapshot_stats, res.snapshot_sample_stats)]
        flat = shard.gather_structured(res.stats, 600, "interleaved")
    finally:
        dist.destroy_process_group()
    for a, b in zip(got, (res.snapshot_stats, res.snapshot_sample_stats)):
        assert a.dtype == abi.STATS_DTYPE and a.shape == (600, len(SNAPS)) and a.tobytes() == b.tobytes()
    assert flat.shape == (600,) and flat.tobytes() == res.stats.tobytes()
