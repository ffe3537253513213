"""End-of-run subsampling fused with the per-replicate ABC statistics (ABI v13; subsample mapping v1) on
the GPU. Final states come from engine.run(spec, want_rows=True) and are first checked against the oracle (event
hash, sorted rows), so the sample is judged on states the oracle vouches for; the samples' statistics and histogram
are compared with the numpy restatement of the mapping (tests/subsample_law.py): integers exactly, floats at the
ABC-statistics tolerance (1e-12 relative: sums are reduced in a different order on the GPU; log is ocml's vs numpy's).
One test checks the law itself, independently of the restatement, against the exact hypergeometric pmf."""
import numpy as np
import pytest

import subsample_law as sl
from ecdna_evo_amd import abi
from exact_law import chi2_lumped
from support.gpu import _flags
from support.subsample_specs import ATOL, BINS, FLOATS, RTOL, STORES, _abc_spec

_ORACLE = {}


def _oracle(oracle_mod, key, spec):
    """One oracle run per final state (the sample size and the target do not change it), shared and left unchanged."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run(spec, want_rows=True)
    return _ORACLE[key]


def _check_state(g, c, spec):
    np.testing.assert_array_equal(g.summaries["event_hash"], c.summaries["event_hash"])
    for f in ("nminus", "nplus", "stop_reason", "error"):
        np.testing.assert_array_equal(g.summaries[f], c.summaries[f])
    for i in range(spec.n_replicates):
        np.testing.assert_array_equal(np.sort(g.row(i)), np.sort(c.row(i)), err_msg=f"row {i}")


def _check_sample(g, spec, tag=""):
    """sample_stats and sample_hist of a run against the restatement applied to the run's own final rows."""
    bins, m = spec.hist_bins, spec.subsample_cells
    tgt = spec.stats_target
    ids = spec.replicate_ids()
    rps = spec.reps_per_set or spec.last_replicate() + 1
    want_hist = np.zeros((len(spec.rates), bins), dtype=np.uint64)
    assert g.sample_stats.dtype == abi.STATS_DTYPE and g.sample_stats.shape == (spec.n_replicates,)
    for i in range(spec.n_replicates):
        nm, row, rid = int(g.summaries[i]["nminus"]), g.row(i), int(ids[i])
        want = sl.sample_stats(nm, row, m, spec.seed, rid, bins, tgt)
        got = g.sample_stats[i]
        assert int(got["cells"]) == want["cells"] == min(m, nm + len(row)), f"{tag} replicate {i}: cells"
        for f in FLOATS:
            np.testing.assert_allclose(got[f], want[f], rtol=RTOL, atol=ATOL, err_msg=f"{tag} replicate {i}: {f}")
        want_hist[rid // rps] += sl.sample_hist(nm, row, m, spec.seed, rid, bins)
    np.testing.assert_array_equal(g.sample_hist, want_hist, err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
@pytest.mark.parametrize("with_target", [False, True])
def test_sample_stats_match_restatement(engine_mod, oracle_mod, with_target, store, kmax):
    """Both stores, every K; sample sizes at, before and after a 64-draw batch edge (63, 64, 65, 128), through the
    complement (1500; 1999 with m' = 1) and the whole population (2000, 4096)."""
    seen_extinct = seen_short = 0
    for m in (1, 63, 64, 65, 128, 700, 1500, 1999, 2000, 4096):
        spec = _abc_spec(store, kmax, with_target, m)
        g = engine_mod.run(spec, want_rows=True)
        _check_state(g, _oracle(oracle_mod, ("abc", store, kmax), spec), spec)
        _check_sample(g, spec, f"m = {m}")
        cells = g.summaries["nminus"] + g.summaries["nplus"]
        seen_extinct += int((cells == 0).sum())
        seen_short += int(((cells > 0) & (cells < m)).sum())
        if m >= 2000:  # the sample is the population: the full statistics, field for field
            for f in FLOATS + ("cells",):
                np.testing.assert_array_equal(g.sample_stats[f], g.stats[f], err_msg=f)
            np.testing.assert_array_equal(g.sample_hist, g.hist)
        if with_target:
            assert np.all(g.sample_stats["ks"][cells == 0] == 1.0)
    assert seen_extinct and seen_short  # N = 0 and early-stopped N < m both occur in this spec


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 32)])
def test_dense_duplicates(engine_mod, oracle_mod, store, kmax):
    """40 positions: the draws of one batch collide with each other, which the kernel must resolve in draw order."""
    dup = 0
    for m in (1, 20, 39):
        spec = abi.RunSpec(seed=12, process=abi.BIRTH_DEATH, rates=((1.0, 1.2, 0.3, 0.3),), n_replicates=512,
                           max_cells=40, hist_bins=33, init={0: 5, 1: 3}, flags=_flags(store), bin_kmax=kmax,
                           subsample_cells=m)
        g = engine_mod.run(spec, want_rows=True)
        _check_state(g, _oracle(oracle_mod, ("dense", store, kmax), spec), spec)
        _check_sample(g, spec, f"m = {m}")
        ids = spec.replicate_ids()
        dup += sum(sl.batch_duplicate(int(g.summaries[i]["nminus"] + g.summaries[i]["nplus"]), m, spec.seed,
                                      int(ids[i])) for i in range(spec.n_replicates))
    assert dup >= 1  # at least one replicate had two equal draws within a batch


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 32)])
def test_population_sizes_around_the_sample_size(engine_mod, oracle_mod, store, kmax):
    """Replicates stopped by MaxTime at 13 to 275 cells, sampled 100 at a time: in one run the whole population
    (N <= 100), the complement with every m' from 1 up (100 < N < 200) and the direct sample (N >= 200)."""
    spec = abi.RunSpec(seed=8, process=abi.BIRTH_DEATH, rates=((1.0, 1.3, 0.4, 0.4),), n_replicates=512, max_cells=3000,
                       max_time=3.0, hist_bins=65, init={0: 6, 1: 4, 70: 2}, flags=_flags(store), bin_kmax=kmax,
                       subsample_cells=100)
    g = engine_mod.run(spec, want_rows=True)
    _check_state(g, _oracle(oracle_mod, ("sizes", store, kmax), spec), spec)
    cells = g.summaries["nminus"] + g.summaries["nplus"]
    assert (cells <= 100).sum() >= 50 and ((cells > 100) & (cells < 200)).sum() >= 50 and (cells >= 200).sum() >= 5
    _check_sample(g, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_limits(engine_mod, oracle_mod, store, kmax):
    """The largest table (m' = 4096 of 8,200 cells) beside the largest histogram (2,048 bins): one wave per workgroup."""
    spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=2048,
                       flags=_flags(store), bin_kmax=kmax, subsample_cells=4096)
    g = engine_mod.run(spec, want_rows=True)
    _check_state(g, _oracle(oracle_mod, ("limits", store, kmax), spec), spec)
    assert np.all(g.summaries["nminus"] + g.summaries["nplus"] == 8200)
    _check_sample(g, spec)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_sample_law_is_hypergeometric(engine_mod, store, kmax):
    """Independent of the restatement: 30 N- and 10 N+ cells, untouched (every replicate stops at MaxCells before its
    first event), sampled 10 at a time: the N+ cells in the sample are Hypergeometric(40, 10, 10)."""
    from scipy import stats

    n = 65536
    spec = abi.RunSpec(seed=2024, process=abi.PURE_BIRTH, n_replicates=n, max_cells=40, hist_bins=17,
                       init={0: 30, 2: 10}, flags=abi.FLAG_REP_STATS | (abi.FLAG_BIN_STORE if store == "bins" else 0),
                       bin_kmax=kmax, subsample_cells=10)
    g = engine_mod.run(spec)
    assert np.all(g.summaries["iters"] == 0) and np.all(g.summaries["nplus"] == 10)
    assert np.all(g.sample_stats["cells"] == 10)
    x = np.rint(g.sample_stats["frequency"] * 10).astype(np.int64)
    np.testing.assert_allclose(g.sample_stats["frequency"] * 10, x, rtol=0, atol=1e-9)
    np.testing.assert_allclose(g.sample_stats["mean"] * 10, 2 * x, rtol=0, atol=1e-9)  # every N+ cell has 2 copies
    obs = np.bincount(x, minlength=11)
    assert len(obs) == 11
    assert int(g.sample_hist[0, 2]) == int(x.sum()) and int(g.sample_hist[0, 0]) == 10 * n - int(x.sum())
    p = chi2_lumped(obs, stats.hypergeom.pmf(np.arange(11), 40, 10, 10) * n, min_expected=5)
    assert p > 1e-6, (p, obs.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_placement_independence(engine_mod, store, kmax, monkeypatch):
    """A replicate's sample depends on its global id only: three interleaved shards, and forced chunks, give the whole
    run's per-replicate sample statistics byte for byte, and their sample histograms sum to the whole run's."""
    whole = engine_mod.run(_abc_spec(store, kmax, True, 700))
    total = np.zeros_like(whole.sample_hist)
    for gi in range(3):
        part = engine_mod.run(_abc_spec(store, kmax, True, 700, first_replicate=gi, replicate_stride=3,
                                        n_replicates=200))
        assert part.sample_stats.tobytes() == whole.sample_stats[gi::3].tobytes(), f"shard {gi}"
        total += part.sample_hist
    np.testing.assert_array_equal(total, whole.sample_hist)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_abc_spec(store, kmax, True, 700)) as ctx:
        assert ctx.instance()["n_chunks"] == 6 and ctx.row_stride() == 0  # rows are not downloadable: the sample is
        ctx.launch()
        ctx.sync()
        chunked = ctx.download()
    assert chunked.sample_stats.tobytes() == whole.sample_stats.tobytes()
    np.testing.assert_array_equal(chunked.sample_hist, whole.sample_hist)
    np.testing.assert_array_equal(chunked.hist, whole.hist)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_nothing_else_moves(engine_mod, store, kmax):
    """With and without subsample_cells every other output is byte-identical; off, there is no sample to download."""
    on = engine_mod.run(_abc_spec(store, kmax, True, 200), want_rows=True)
    with engine_mod.Context(_abc_spec(store, kmax, True, 0)) as ctx:
        ctx.launch()
        ctx.sync()
        off = ctx.download(want_rows=True)
        st = np.zeros(600, dtype=abi.STATS_DTYPE)
        rc = engine_mod.lib().ecdna_ssa_ctx_download_sample(ctx.h, st.ctypes.data, None)
        assert rc == abi.E_STATE and engine_mod.lib().ecdna_ssa_last_error_message()
    assert off.sample_stats is None and off.sample_hist is None
    assert on.sample_stats is not None and on.sample_hist.shape == (2, BINS)
    for a, b in ((on.summaries, off.summaries), (on.totals, off.totals), (on.stats, off.stats), (on.hist, off.hist)):
        assert a.tobytes() == b.tobytes()
    for i in range(600):
        np.testing.assert_array_equal(on.row(i), off.row(i))
    # before a launch there is nothing to download either
    with engine_mod.Context(_abc_spec(store, kmax, True, 200)) as ctx:
        assert engine_mod.lib().ecdna_ssa_ctx_download_sample(ctx.h, None, None) == abi.E_STATE
        ctx.launch()
        assert engine_mod.lib().ecdna_ssa_ctx_download_sample(ctx.h, None, None) == abi.OK  # both buffers may be NULL


@pytest.mark.gpu
def test_gather_structured_takes_sample_stats(engine_mod, tmp_path):
    """shard.gather_structured moves any STATS_DTYPE array as raw bytes: the samples' statistics come back bit for bit
    (a one-rank gloo group in this process; tests/test_gpu_abc_gather.py runs the exchange across ranks)."""
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    res = engine_mod.run(_abc_spec("bins", 64, True, 128))
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        got = shard.gather_structured(res.sample_stats, 600, "interleaved")
    finally:
        dist.destroy_process_group()
    assert got.dtype == abi.STATS_DTYPE and got.tobytes() == res.sample_stats.tobytes()
