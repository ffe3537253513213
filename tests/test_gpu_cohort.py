"""One sweep scored against a cohort of targets on the GPU (ecdna_ssa_cohort_t, cohort mapping v1; include/ecdna_ssa.h,
DESIGN.md §3.4).

The reference everywhere is the existing single-target path of the same build, which tests/test_gpu_abc_stats.py and
tests/test_gpu_subsample_stats.py pin to the numpy restatements: cohort.stats[p] and cohort.sample_stats[p] must be, byte
for byte, the stats and sample_stats of the plain run with stats_target = H_p and subsample_cells = m_p. The spec is
that of tests/test_gpu_subsample_stats.py (birth-death, two sets of 300 replicates to 2,000 cells, a 300-copy cell so
that the large-k row and the overflow bin are used; both stores, every K). The plain runs are made once per store and
shared, unchanged, by the tests that need them."""
import ctypes as C

import numpy as np
import pytest

import abc_stats
import subsample_law as sl
from ecdna_evo_amd import abi
from support.cohort_specs import P, SAMPLE_CELLS, _targets
from support.gpu import _flags, _launched, _same_accept, _same_select, _thresholds
from support.subsample_specs import ATOL, BINS, FLOATS, RTOL, STORES, _abc_spec

INF = np.inf
OWN_M = 200  # the cohort run's own params.subsample_cells: it keeps its meaning beside the block
_PLAIN = {}
_COHORT = {}


def _cohort_spec(store, kmax, sample_cells=SAMPLE_CELLS, block=True, **kw):
    """The spec with its own target (target 0) and its own sample size, and — block — the cohort of all six."""
    t = _targets()
    spec = _abc_spec(store, kmax, True, OWN_M, **kw)
    spec.stats_target = t[0]
    if block:
        spec.cohort_targets = t
        spec.cohort_sample_cells = sample_cells
    return spec


def _plain(engine_mod, store, kmax, p):
    """The plain run against target p with p's sample size: one per (store, p), shared and left unchanged."""
    key = (store, kmax, p)
    if key not in _PLAIN:
        spec = _abc_spec(store, kmax, True, SAMPLE_CELLS[p])
        spec.stats_target = _targets()[p]
        _PLAIN[key] = engine_mod.run(spec)
    return _PLAIN[key]


def _cohort(engine_mod, store, kmax):
    key = (store, kmax)
    if key not in _COHORT:
        _COHORT[key] = engine_mod.run(_cohort_spec(store, kmax), want_rows=True)
    return _COHORT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
def test_cohort_equals_the_plain_runs_byte_for_byte(engine_mod, store, kmax):
    g = _cohort(engine_mod, store, kmax)
    co = g.cohort
    assert co.stats.dtype == abi.STATS_DTYPE and co.stats.shape == co.sample_stats.shape == (P, 600)
    cells = g.summaries["nminus"] + g.summaries["nplus"]
    # the spec's hard cases occur: extinct replicates, and populations smaller than a sample size
    assert (cells == 0).sum() and ((cells > 0) & (cells < max(SAMPLE_CELLS))).sum()
    assert ((cells > 1500) & (cells < 3000)).sum()  # ... and the complement: 1500 cells by the N - 1500 < 1500 left out
    for p in range(P):
        plain = _plain(engine_mod, store, kmax, p)
        np.testing.assert_array_equal(plain.summaries["event_hash"], g.summaries["event_hash"])  # the same run
        for f in FLOATS + ("cells",):  # (named fields first: a failure says which)
            np.testing.assert_array_equal(co.stats[p][f].view(np.uint64), plain.stats[f].view(np.uint64),
                                          err_msg=f"target {p}: stats.{f}")
            np.testing.assert_array_equal(co.sample_stats[p][f].view(np.uint64), plain.sample_stats[f].view(np.uint64),
                                          err_msg=f"target {p}: sample_stats.{f}")
        assert co.stats[p].tobytes() == plain.stats.tobytes(), f"target {p}"
        assert co.sample_stats[p].tobytes() == plain.sample_stats.tobytes(), f"target {p}"
        assert np.all(co.stats[p]["ks"][cells == 0] == 1.0) and np.all(co.sample_stats[p]["ks"][cells == 0] == 1.0)
        assert np.all(co.sample_stats[p]["cells"] == np.minimum(cells, SAMPLE_CELLS[p]))
        for f in ("mean", "entropy", "frequency", "cells"):  # target-independent
            assert co.stats[p][f].tobytes() == co.stats[0][f].tobytes()
    # two targets with equal m see the same sample; the distances tell the targets apart
    for f in ("mean", "entropy", "frequency", "cells"):
        assert co.sample_stats[0][f].tobytes() == co.sample_stats[3][f].tobytes()
    assert co.sample_stats[0]["ks"].tobytes() != co.sample_stats[3]["ks"].tobytes()
    assert co.stats[0]["ks"].tobytes() != co.stats[1]["ks"].tobytes()
    # the whole population as the sample (m = 4096): the full record against the same target
    assert co.sample_stats[4].tobytes() == co.stats[4].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
def test_one_target_against_the_restatement(engine_mod, store, kmax):
    """Target 1 (the complement, m = 1500) against tests/subsample_law.py and oracle/abc_stats.py on the run's own rows."""
    p, g = 1, _cohort(engine_mod, store, kmax)
    tgt, ids = _targets()[p], _cohort_spec(store, kmax).replicate_ids()
    for i in range(600):
        nm, row = int(g.summaries[i]["nminus"]), g.row(i)
        want_full = abc_stats.rep_stats(nm, row, BINS, tgt)
        want = sl.sample_stats(nm, row, SAMPLE_CELLS[p], 4, int(ids[i]), BINS, tgt)
        assert int(g.cohort.stats[p][i]["cells"]) == want_full["cells"] == nm + len(row)
        assert int(g.cohort.sample_stats[p][i]["cells"]) == want["cells"]
        for f in FLOATS:
            np.testing.assert_allclose(g.cohort.stats[p][i][f], want_full[f], rtol=RTOL, atol=ATOL,
                                       err_msg=f"replicate {i}: stats.{f}")
            np.testing.assert_allclose(g.cohort.sample_stats[p][i][f], want[f], rtol=RTOL, atol=ATOL,
                                       err_msg=f"replicate {i}: sample_stats.{f}")


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_placement_independence(engine_mod, store, kmax, monkeypatch):
    """200 replicates in one chunk, in forced chunks (rows not downloadable), and as two interleaved shards."""
    whole = engine_mod.run(_cohort_spec(store, kmax, n_replicates=200)).cohort
    for g in range(2):
        part = engine_mod.run(_cohort_spec(store, kmax, first_replicate=g, replicate_stride=2, n_replicates=100)).cohort
        for p in range(P):
            assert part.stats[p].tobytes() == whole.stats[p][g::2].tobytes(), (g, p)
            assert part.sample_stats[p].tobytes() == whole.sample_stats[p][g::2].tobytes(), (g, p)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_cohort_spec(store, kmax, n_replicates=200)) as ctx:
        assert ctx.instance()["n_chunks"] == 2 and ctx.row_stride() == 0
        ctx.launch()
        ctx.sync()
        chunked = ctx.download().cohort
    assert chunked.stats.tobytes() == whole.stats.tobytes()
    assert chunked.sample_stats.tobytes() == whole.sample_stats.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_through_accept_and_select(engine_mod, store, kmax, tmp_path):
    """Timepoint p of the cohort sources is plain run p: the same acceptance, the same order statistics."""
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    fractions, ranks = (0.01, 0.1, 0.5, 1.0), (1, 2, 300, 599, 600, 601)
    masks = []
    with _launched(engine_mod, _cohort_spec(store, kmax)) as ctx:
        res = ctx.download()
        assert ctx.accept_timepoints(abi.ACCEPT_COHORT) == ctx.accept_timepoints(abi.ACCEPT_COHORT_SAMPLES) == P
        thr0 = None
        for p in range(P):
            spec = _abc_spec(store, kmax, True, SAMPLE_CELLS[p])
            spec.stats_target = _targets()[p]
            with _launched(engine_mod, spec) as plain:
                pres = plain.download()
                # the run's own order statistics as thresholds, so that ties on the boundary occur
                thr = _thresholds(pres.sample_stats[:, None], pres.summaries)
                thr0 = thr if thr0 is None else thr0
                for q, cap in ((0, 0), (2, 50), (5, 600)):
                    want = plain.accept(abi.ACCEPT_SAMPLE, thr, None, q, cap)
                    got = ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr, [p], q, cap)
                    _same_accept(got, want, f"samples, target {p}, row {q}")
                    assert got.stats.shape == (len(want.ids), P)  # all P records of each listed replicate
                    assert np.ascontiguousarray(got.stats[:, p]).tobytes() == want.stats[:, 0].tobytes()
                    listed = got.ids.astype(np.int64)  # (ids 0 .. 599: the id is the index)
                    assert got.stats.tobytes() == np.ascontiguousarray(res.cohort.sample_stats[:, listed].T).tobytes()
                per_row = want.counts.sum(axis=1)
                # (rows 0 .. 4: the 10 % .. 90 % order statistics of each distance, row 5: all inf) no row is trivial
                assert 0 < per_row[4] and per_row[0] < per_row[5] == (pres.summaries["error"] == 0).sum()
                thr_full = _thresholds(pres.stats[:, None], pres.summaries)
                _same_accept(ctx.accept(abi.ACCEPT_COHORT, thr_full, [p], 1, 600),
                             plain.accept(abi.ACCEPT_FINAL, thr_full, None, 1, 600), f"full, target {p}")
                for kw in (dict(fractions=fractions), dict(ranks=ranks)):
                    _same_select(ctx.select(abi.ACCEPT_COHORT_SAMPLES, timepoints=[p], **kw),
                                 plain.select(abi.ACCEPT_SAMPLE, **kw), f"samples, target {p}")
                    _same_select(ctx.select(abi.ACCEPT_COHORT, timepoints=[p], **kw),
                                 plain.select(abi.ACCEPT_FINAL, **kw), f"full, target {p}")
            masks.append(ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr0, [p]).mask)
        # all P jointly (mask 0): a replicate passes a row iff it passes it for every target
        joint = ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr0)
        np.testing.assert_array_equal(joint.mask, np.bitwise_and.reduce(np.stack(masks), axis=0))
        assert joint.counts[5].sum() == (res.summaries["error"] == 0).sum() > joint.counts[4].sum()
        # two interleaved shards: the counts sum, and the digit histograms walk to the whole run's order statistics
        total = np.zeros_like(joint.counts)
        walk = shard.SelectWalk(len(fractions), fractions=fractions)
        parts = [_launched(engine_mod, _cohort_spec(store, kmax, first_replicate=g, replicate_stride=2,
                                                    n_replicates=300)) for g in range(2)]
        try:
            for part in parts:
                total += part.accept(abi.ACCEPT_COHORT_SAMPLES, thr0, [1, 5]).counts
            for ps in range(shard.SelectWalk.PASSES):
                walk.feed(sum(part.select_digits(abi.ACCEPT_COHORT_SAMPLES, ps, walk.prefixes, [1, 5])
                              for part in parts))
        finally:
            for part in parts:
                part.close()
        np.testing.assert_array_equal(total, ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr0, [1, 5]).counts)
        want = ctx.select(abi.ACCEPT_COHORT_SAMPLES, fractions=fractions, timepoints=[1, 5])
        _same_select(walk.result(), want, "two shards")
        # shard.select over a process group of one
        assert not dist.is_initialized()
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            got = shard.select(ctx, abi.ACCEPT_COHORT_SAMPLES, fractions=fractions, timepoints=[1, 5])
        finally:
            dist.destroy_process_group()
        _same_select(got, want, "shard.select")


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_nothing_else_moves(engine_mod, store, kmax):
    """With the block every other output is that of the same spec without it; without it there is nothing to download."""
    L = engine_mod.lib()
    on = _cohort(engine_mod, store, kmax)
    thr = np.asarray([[INF] * 4])
    with engine_mod.Context(_cohort_spec(store, kmax)) as ctx:
        ins_on = ctx.instance()
        assert L.ecdna_ssa_ctx_download_cohort(ctx.h, None, None) == abi.E_STATE  # before a launch
    with engine_mod.Context(_cohort_spec(store, kmax, block=False)) as ctx:
        assert ctx.instance() == ins_on
        ctx.launch()
        ctx.sync()
        off = ctx.download(want_rows=True)
        st = np.zeros((P, 600), dtype=abi.STATS_DTYPE)
        assert L.ecdna_ssa_ctx_download_cohort(ctx.h, st.ctypes.data, None) == abi.E_STATE
        assert b"cohort" in L.ecdna_ssa_last_error_message()
        with pytest.raises(engine_mod.EngineError):
            ctx.download_cohort()
        for source in (abi.ACCEPT_COHORT, abi.ACCEPT_COHORT_SAMPLES):
            a = abi.Accept(struct_size=C.sizeof(abi.Accept), source=source, n_thresholds=1)
            a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
            assert L.ecdna_ssa_ctx_accept(ctx.h, C.byref(a)) == abi.E_STATE, source
            rk = (C.c_uint64 * 1)(1)
            s = abi.Select(struct_size=C.sizeof(abi.Select), source=source, n_ranks=1)
            s.ranks = C.cast(rk, C.POINTER(C.c_uint64))
            assert L.ecdna_ssa_ctx_select(ctx.h, C.byref(s), None, None, None, None) == abi.E_STATE, source
            hist = np.zeros((4, 1, 256), dtype=np.uint64)
            pre = np.zeros((4, 1), dtype=np.uint64)
            assert L.ecdna_ssa_ctx_select_digits(ctx.h, source, 0, 0, 1, pre.ctypes.data, hist.ctypes.data) == abi.E_STATE
    assert off.cohort is None and on.cohort is not None
    for name in ("summaries", "hist", "totals", "stats", "sample_stats", "sample_hist"):
        assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
    assert np.all(on.sample_stats["cells"] == np.minimum(on.summaries["nminus"] + on.summaries["nplus"], OWN_M))
    for i in range(600):
        np.testing.assert_array_equal(on.row(i), off.row(i))
    # without sample sizes: the full records alone
    with _launched(engine_mod, _cohort_spec(store, kmax, sample_cells=None)) as ctx:
        res = ctx.download()
        assert res.cohort.sample_stats is None and res.cohort.stats.tobytes() == on.cohort.stats.tobytes()
        st = np.zeros((P, 600), dtype=abi.STATS_DTYPE)
        assert L.ecdna_ssa_ctx_download_cohort(ctx.h, st.ctypes.data, st.ctypes.data) == abi.E_STATE
        assert b"sample_cells" in L.ecdna_ssa_last_error_message()
        assert L.ecdna_ssa_ctx_download_cohort(ctx.h, st.ctypes.data, None) == abi.OK
        assert st.tobytes() == on.cohort.stats.tobytes()
        with pytest.raises(engine_mod.EngineError, match="sample_cells"):
            ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr)
        with pytest.raises(engine_mod.EngineError, match="sample_cells"):
            ctx.select(abi.ACCEPT_COHORT_SAMPLES, ranks=[1])
        assert ctx.accept(abi.ACCEPT_COHORT, thr).counts.sum() == ctx.select(abi.ACCEPT_COHORT, ranks=[1]).population
        # 6 and 7 are not sources
        for source in (6, 7, 10):
            with pytest.raises(engine_mod.EngineError, match="source"):
                ctx.accept(source, thr)
            with pytest.raises(engine_mod.EngineError, match="source"):
                ctx.select(source, ranks=[1])
            pre = np.zeros((4, 1), dtype=np.uint64)
            hist = np.zeros((4, 1, 256), dtype=np.uint64)
            assert L.ecdna_ssa_ctx_select_digits(ctx.h, source, 0, 0, 1, pre.ctypes.data, hist.ctypes.data) == abi.E_INVALID
            assert b"source" in L.ecdna_ssa_last_error_message()
        # a timepoint at or above P
        with pytest.raises(engine_mod.EngineError, match="timepoint_mask"):
            ctx.accept(abi.ACCEPT_COHORT, thr, [P])


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_limits(engine_mod, store, kmax):
    """The largest table beside the largest histogram, P = 64: m = 4096 for every target but one at 4095 (two groups at
    the largest table), 64 pure-birth replicates of 8,200 cells. Targets 0 and 63 against their plain runs."""
    bins, n_targets = 2048, 64
    rng = np.random.default_rng(9)
    targets = rng.integers(0, 50, (n_targets, bins)).astype(np.uint64)
    targets[:, 0] += 1
    cells = [4096] * n_targets
    cells[63] = 4095
    base = dict(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=bins, flags=_flags(store),
                bin_kmax=kmax)
    g = engine_mod.run(abi.RunSpec(cohort_targets=targets, cohort_sample_cells=cells, **base))
    assert np.all(g.summaries["nminus"] + g.summaries["nplus"] == 8200)
    for p in (0, 63):
        plain = engine_mod.run(abi.RunSpec(stats_target=targets[p], subsample_cells=cells[p], **base))
        assert g.cohort.stats[p].tobytes() == plain.stats.tobytes(), p
        assert g.cohort.sample_stats[p].tobytes() == plain.sample_stats.tobytes(), p
        assert np.all(g.cohort.sample_stats[p]["cells"] == cells[p])
    assert g.cohort.sample_stats[0]["mean"].tobytes() == g.cohort.sample_stats[62]["mean"].tobytes()
    assert g.cohort.sample_stats[0]["mean"].tobytes() != g.cohort.sample_stats[63]["mean"].tobytes()
