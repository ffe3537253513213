"""Every replicate's sample kept on the GPU, scored and pooled after the sweep (ecdna_ssa_keep_t, keep mapping v1;
include/ecdna_ssa.h).

Every comparison is exact. The kept samples are compared with the numpy restatement (tests/keep_law.py on top of
tests/subsample_law.py) applied to the run's own rows; the rescored records with the launch-time paths of the same build
(the cohort block's sample records and the plain run's, which tests/test_gpu_cohort.py and
tests/test_gpu_subsample_stats.py pin to the restatements) as bytes; accept and select over the rescored records with
tests/accept_law.py and tests/select_law.py on the downloaded records; the pooled histogram with keep_law.pooled of the
downloaded kept samples and mask. The spec is that of tests/test_gpu_subsample_stats.py (birth-death, two sets of 300
replicates to 2,000 cells, a 300-copy cell, 257 bins)."""
import numpy as np
import pytest

import accept_law as al
import keep_law as kl
import select_law as slw
from ecdna_evo_amd import abi
from support.cohort_specs import _targets
from support.gpu import ALL_INF_ROW, _canon, _flags, _launched, _same_accept, _same_select, _source_codes, _thresholds
from support.subsample_specs import BINS, STORES, _abc_spec

INF = np.inf
P = 6  # support.cohort_specs._targets()
OWN_M = 200  # the run's own params.subsample_cells: it keeps its meaning beside the block
SEED = 4  # _abc_spec's
TWO_STORES = [("rows", 0), ("bins", 64)]
FRACTIONS, RANKS = (0.01, 0.1, 0.5, 1.0), (1, 2, 300, 599, 600, 601)
_PLAIN = {}


def _keep_spec(store, kmax, m, cohort_m=None, **kw):
    """The spec with its own target (target 0) and its own sample size, the keep block of m cells (None: no block) and
    — cohort_m — the cohort of all six targets, each with cohort_m cells."""
    t = _targets()
    spec = _abc_spec(store, kmax, True, OWN_M, **kw)
    spec.stats_target = t[0]
    spec.keep_cells = m
    if cohort_m is not None:
        spec.cohort_targets = t
        spec.cohort_sample_cells = (cohort_m,) * P
    return spec


def _plain(engine_mod, store, kmax, p, m):
    """The plain run against target p with subsample_cells = m: one per key, shared and left unchanged."""
    key = (store, kmax, p, m)
    if key not in _PLAIN:
        spec = _abc_spec(store, kmax, True, m)
        spec.stats_target = _targets()[p]
        _PLAIN[key] = engine_mod.run(spec)
    return _PLAIN[key]


def _hard_cases_occur(summaries):
    cells = summaries["nminus"] + summaries["nplus"]
    # extinct replicates, populations smaller than a sample (of 4096 cells), and the complement at m = 1500 (N - 1500 <
    # 1500 left out): what tests/test_gpu_cohort.py asserts of this seed
    assert (cells == 0).sum() and ((cells > 0) & (cells < 4096)).sum() and ((cells > 1500) & (cells < 3000)).sum()
    return cells


def _check_kept(engine_mod, store, kmax, m):
    spec = _keep_spec(store, kmax, m)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download(want_rows=True)
        headers, cells = ctx.download_kept()
    assert headers.dtype == abi.KEPT_DTYPE and headers.shape == (600,) and cells.shape == (600, m)
    pop = _hard_cases_occur(res.summaries)
    ids = spec.replicate_ids()
    for i in range(600):
        want_h, want_c = kl.kept(int(res.summaries[i]["nminus"]), res.row(i), m, SEED, int(ids[i]))
        assert (int(headers[i]["nminus"]), int(headers[i]["nplus"])) == want_h, (m, i)
        np.testing.assert_array_equal(cells[i, :want_h[1]], want_c, err_msg=f"m = {m}, replicate {i}")
    assert np.all(headers["nminus"].astype(np.int64) + headers["nplus"] == np.minimum(pop, m))
    assert np.all(headers["nminus"][pop == 0] == 0) and np.all(headers["nplus"][pop == 0] == 0)  # the empty sample
    return headers, cells


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", STORES)
def test_kept_samples_against_the_law(engine_mod, store, kmax):
    """Headers and cells of all 600 replicates at m = 64 (the picks) and m = 1500 (picks, complement, whole)."""
    for m in (64, 1500):
        _check_kept(engine_mod, store, kmax, m)


@pytest.mark.gpu
def test_kept_samples_at_the_edges(engine_mod):
    """m = 1, the batch edge m = 65, and m = 4096, where the whole population is kept; the true copy number is kept, not
    the clipped bin."""
    for m in (1, 65):
        _check_kept(engine_mod, "bins", 64, m)
    headers, cells = _check_kept(engine_mod, "bins", 64, 4096)
    inside = np.arange(4096)[None, :] < headers["nplus"].astype(np.int64)[:, None]
    assert ((cells == 300) & inside).any() and BINS - 1 < 300


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("m", [64, 1500, 4096])
def test_rescored_records_equal_the_launch_time_records(engine_mod, store, kmax, m):
    t = _targets()
    with _launched(engine_mod, _keep_spec(store, kmax, m, cohort_m=m)) as ctx:
        res = ctx.download()
        got = ctx.rescore(t)
        assert got.dtype == abi.STATS_DTYPE and got.shape == (P, 600)
        assert ctx.download_rescored().tobytes() == got.tobytes()
        assert ctx.accept_timepoints(abi.ACCEPT_RESCORED) == P
    _hard_cases_occur(res.summaries)
    want = res.cohort.sample_stats
    for p in range(P):
        for f in abi.STATS_DTYPE.names:  # (named fields first: a failure says which)
            np.testing.assert_array_equal(got[p][f].view(np.uint64), want[p][f].view(np.uint64),
                                          err_msg=f"target {p}: {f}")
    assert got.tobytes() == want.tobytes()
    plain = _plain(engine_mod, store, kmax, 1, m)
    np.testing.assert_array_equal(plain.summaries["event_hash"], res.summaries["event_hash"])  # the same run
    assert got[1].tobytes() == plain.sample_stats.tobytes()


@pytest.mark.gpu
def test_a_second_rescore_replaces_the_first(engine_mod):
    """P = 1 with target 2 (mass only in bin 0), then P = 6: download, accept and select on the same timepoint mask
    answer from the second call's records — a stale key cache of the select would answer from the first's."""
    t = _targets()
    spec = _keep_spec("bins", 64, 64)
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        first = ctx.rescore(t[2:3])
        assert first.shape == (1, 600) and ctx.accept_timepoints(abi.ACCEPT_RESCORED) == 1
        sel_first = ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS, timepoints=[0])
        acc_first = ctx.accept(abi.ACCEPT_RESCORED, _thresholds(first[0][:, None], summ), [0])
        with pytest.raises(engine_mod.EngineError, match="timepoint_mask"):
            ctx.accept(abi.ACCEPT_RESCORED, [[INF] * 4], [1])  # T is the P of the last rescore
        second = ctx.rescore(t)
        assert second.shape == (P, 600) and ctx.download_rescored().tobytes() == second.tobytes()
        assert second[2].tobytes() == first[0].tobytes() and second[0].tobytes() != first[0].tobytes()
        records = np.ascontiguousarray(second.T)  # [n][P]
        thr = _thresholds(second[0][:, None], summ)  # the run's own order statistics: ties on the boundary occur
        for kw in (dict(fractions=FRACTIONS), dict(ranks=RANKS)):
            got = ctx.select(abi.ACCEPT_RESCORED, timepoints=[0], **kw)
            _same_select(got, slw.select(records, summ, timepoint_mask=1, **kw), "after the second rescore")
        assert got.population == (summ["error"] == 0).sum()
        now = ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS, timepoints=[0])
        assert now.values.tobytes() != sel_first.values.tobytes()  # (the two targets' order statistics differ)
        for q, cap in ((0, 0), (2, 50), (ALL_INF_ROW, 600)):
            got = ctx.accept(abi.ACCEPT_RESCORED, thr, [0], q, cap)
            want = al.accept(records, summ, 300, spec.replicate_ids(), thr, 2, 1, q, cap)
            _same_accept(got, want, f"row {q}")
            assert got.stats.shape == (len(want.ids), P)
            assert got.stats.tobytes() == records[want.index].tobytes()
        per_row = got.counts.sum(axis=1)
        assert 0 < per_row[4] and per_row[0] < per_row[ALL_INF_ROW] == (summ["error"] == 0).sum()
        assert not np.array_equal(ctx.accept(abi.ACCEPT_RESCORED, thr, [0]).mask, acc_first.mask)
        # all six jointly, and a later P = 1 again
        _same_accept(ctx.accept(abi.ACCEPT_RESCORED, thr), al.accept(records, summ, 300, spec.replicate_ids(), thr, 2),
                     "all targets")
        third = ctx.rescore(t[2:3])
        assert third.tobytes() == first.tobytes()
        _same_select(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS, timepoints=[0]), sel_first, "third rescore")


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_through_accept_and_select(engine_mod, store, kmax):
    """Timepoint p of the rescored records is timepoint p of the cohort's sample records on the same context."""
    m = 64
    with _launched(engine_mod, _keep_spec(store, kmax, m, cohort_m=m)) as ctx:
        res = ctx.download()
        rec = ctx.rescore(_targets())
        for p in range(P):
            thr = _thresholds(rec[p][:, None], res.summaries)
            for q, cap in ((0, 0), (2, 50), (ALL_INF_ROW, 600)):
                got = ctx.accept(abi.ACCEPT_RESCORED, thr, [p], q, cap)
                want = ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr, [p], q, cap)
                _same_accept(got, want, f"target {p}, row {q}")
                assert got.stats.tobytes() == want.stats.tobytes()
            per_row = want.counts.sum(axis=1)
            assert 0 < per_row[4] and per_row[0] < per_row[ALL_INF_ROW]
            for kw in (dict(fractions=FRACTIONS), dict(ranks=RANKS)):
                _same_select(ctx.select(abi.ACCEPT_RESCORED, timepoints=[p], **kw),
                             ctx.select(abi.ACCEPT_COHORT_SAMPLES, timepoints=[p], **kw), f"target {p}")
        thr = _thresholds(rec[0][:, None], res.summaries)
        _same_accept(ctx.accept(abi.ACCEPT_RESCORED, thr, [1, 5]), ctx.accept(abi.ACCEPT_COHORT_SAMPLES, thr, [1, 5]),
                     "two targets jointly")
        hist = [ctx.select_digits(src, 0, np.zeros((4, 1), dtype=np.uint64), [3])
                for src in (abi.ACCEPT_RESCORED, abi.ACCEPT_COHORT_SAMPLES)]
        np.testing.assert_array_equal(hist[0], hist[1])


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_pooled_accepted_histogram(engine_mod, store, kmax, tmp_path):
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    m, t = 64, _targets()
    spec = _keep_spec(store, kmax, m)
    sets = (spec.replicate_ids() // np.uint64(300)).astype(np.int64)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download()
        headers, cells = ctx.download_kept()
        rec = ctx.rescore(t)
        thr = _thresholds(rec[0][:, None], res.summaries)
        acc = ctx.accept(abi.ACCEPT_RESCORED, thr, [0])
        whole = {}
        for q in (0, 2, ALL_INF_ROW):
            got = ctx.pool_accepted(q)
            assert got.dtype == np.uint64 and got.shape == (2, BINS)
            np.testing.assert_array_equal(got, kl.pooled(headers, cells, acc.mask, q, sets, BINS, 2), err_msg=f"row {q}")
            on = ((acc.mask >> np.uint32(q)) & 1).astype(bool)
            assert on.sum() == acc.counts[q].sum()
            for s in range(2):
                mine = on & (sets == s)
                assert got[s].sum() == (headers["nminus"][mine].astype(np.int64) + headers["nplus"][mine]).sum()
            whole[q] = got
        assert whole[0].sum() <= whole[2].sum() < whole[ALL_INF_ROW].sum() and whole[2].sum() > 0
        # the all-inf row pools every error-free replicate's sample: the run's own sample histogram at the same m
        if not (res.summaries["error"] != 0).any():
            plain = _plain(engine_mod, store, kmax, 1, m)
            np.testing.assert_array_equal(whole[ALL_INF_ROW], plain.sample_hist)
        # whatever the source of the accept: the run's own full statistics
        thr_full = _thresholds(res.stats[:, None], res.summaries)
        acc_full = ctx.accept(abi.ACCEPT_FINAL, thr_full)
        np.testing.assert_array_equal(ctx.pool_accepted(1), kl.pooled(headers, cells, acc_full.mask, 1, sets, BINS, 2))
        # a row that accepts nothing: ks = 0 against target 4, which has mass only in the overflow bin
        none = ctx.accept(abi.ACCEPT_RESCORED, [[0.0, INF, INF, INF]], [4])
        assert none.counts.sum() == 0 and not ctx.pool_accepted(0).any()
        with pytest.raises(engine_mod.EngineError, match="threshold"):
            ctx.pool_accepted(1)  # that accept had one row
        # two interleaved shards' arrays sum to the whole run's
        ctx.accept(abi.ACCEPT_RESCORED, thr, [0])
        total = np.zeros((2, BINS), dtype=np.uint64)
        for g in range(2):
            with _launched(engine_mod, _keep_spec(store, kmax, m, first_replicate=g, replicate_stride=2,
                                                  n_replicates=300)) as part:
                part.rescore(t)
                part.accept(abi.ACCEPT_RESCORED, thr, [0])
                total += part.pool_accepted(2)
        np.testing.assert_array_equal(total, whole[2])
        # shard.pool_accepted over a process group of one
        assert not dist.is_initialized()
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            got = shard.pool_accepted(ctx, 2)
        finally:
            dist.destroy_process_group()
        np.testing.assert_array_equal(got, whole[2])


@pytest.mark.gpu
def test_download_kept_by_ids(engine_mod):
    m, t = 65, _targets()
    L = engine_mod.lib()
    with _launched(engine_mod, _keep_spec("rows", 0, m)) as ctx:
        res = ctx.download()
        headers, cells = ctx.download_kept()
        rec = ctx.rescore(t)
        acc = ctx.accept(abi.ACCEPT_RESCORED, _thresholds(rec[0][:, None], res.summaries), [0], 3, 600)
        assert 1 < len(acc.ids) < 600
        ids = acc.ids[::-1].copy()
        got_h, got_c = ctx.download_kept(ids=ids)
        index = ids.astype(np.int64)  # (ids 0 .. 599: the id is the index)
        assert got_h.shape == (len(ids),) and got_c.shape == (len(ids), m)
        assert _canon(got_h, got_c) == _canon(headers[index], cells[index])
        h5, c5 = ctx.download_kept(count=5)
        assert _canon(h5, c5) == _canon(headers[:5], cells[:5])
        # an id outside the call; more than the call's replicates
        out_h, out_c = np.zeros(2, dtype=abi.KEPT_DTYPE), np.zeros((2, m), dtype=np.uint16)
        bad = np.asarray([5, 600], dtype=np.uint64)
        assert L.ecdna_ssa_ctx_download_kept(ctx.h, 2, bad.ctypes.data, out_h.ctypes.data, out_c.ctypes.data) == abi.E_INVALID
        assert b"ids[1]" in L.ecdna_ssa_last_error_message()
        assert L.ecdna_ssa_ctx_download_kept(ctx.h, 601, None, None, None) == abi.E_INVALID
    with _launched(engine_mod, _keep_spec("rows", 0, m, first_replicate=1, replicate_stride=2, n_replicates=300)) as part:
        ids = np.asarray([599, 1, 301], dtype=np.uint64)
        got_h, got_c = part.download_kept(ids=ids)
        assert _canon(got_h, got_c) == _canon(headers[[599, 1, 301]], cells[[599, 1, 301]])
        for bad_id in (2, 0, 601):  # off the stride, before the first, past the last
            bad = np.asarray([1, bad_id], dtype=np.uint64)
            assert L.ecdna_ssa_ctx_download_kept(part.h, 2, bad.ctypes.data, out_h.ctypes.data,
                                                 out_c.ctypes.data) == abi.E_INVALID, bad_id


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_placement_independence(engine_mod, store, kmax, monkeypatch):
    """200 replicates in one chunk, as two interleaved shards, and in forced chunks (rows not downloadable)."""
    m, t = 1500, _targets()

    def outputs(ctx):
        headers, cells = ctx.download_kept()
        return headers, cells, ctx.rescore(t)

    with _launched(engine_mod, _keep_spec(store, kmax, m, n_replicates=200)) as ctx:
        headers, cells, rec = outputs(ctx)
    assert (headers["nplus"] > 0).sum() > 100
    for g in range(2):
        with _launched(engine_mod, _keep_spec(store, kmax, m, first_replicate=g, replicate_stride=2,
                                              n_replicates=100)) as part:
            ph, pc, prec = outputs(part)
        assert _canon(ph, pc) == _canon(headers[g::2], cells[g::2]), g
        for p in range(P):
            assert prec[p].tobytes() == rec[p][g::2].tobytes(), (g, p)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_keep_spec(store, kmax, m, n_replicates=200)) as ctx:
        assert ctx.instance()["n_chunks"] == 2 and ctx.row_stride() == 0
        ctx.launch()
        ctx.sync()
        ch, cc, crec = outputs(ctx)
    assert _canon(ch, cc) == _canon(headers, cells)
    assert crec.tobytes() == rec.tobytes()


def _raw_calls(L, h, n, m):
    """The return codes of the four calls over the kept samples, with arguments that are valid on a keep context."""
    hists = np.ones((1, BINS), dtype=np.uint64)
    rec = np.zeros((1, n), dtype=abi.STATS_DTYPE)
    pool = np.zeros((2, BINS), dtype=np.uint64)
    kh, kc = np.zeros(n, dtype=abi.KEPT_DTYPE), np.zeros((n, max(m, 1)), dtype=np.uint16)
    return (L.ecdna_ssa_ctx_rescore(h, 1, hists.ctypes.data), L.ecdna_ssa_ctx_download_rescored(h, rec.ctypes.data),
            L.ecdna_ssa_ctx_pool_accepted(h, 0, pool.ctypes.data),
            L.ecdna_ssa_ctx_download_kept(h, n, None, kh.ctypes.data, kc.ctypes.data))


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_nothing_else_moves(engine_mod, store, kmax):
    """With the block every other output is that of the same spec without it; without it, before a launch and after a
    relaunch the new calls say so."""
    L = engine_mod.lib()
    m, E = 64, abi.E_STATE
    with engine_mod.Context(_keep_spec(store, kmax, m)) as ctx:
        ins_on = ctx.instance()
        assert _raw_calls(L, ctx.h, 600, m) == (E, E, E, E)  # before a launch
        assert _source_codes(L, ctx.h, abi.ACCEPT_RESCORED) == (E, E, E)
        ctx.launch()
        ctx.sync()
        on = ctx.download(want_rows=True)
        assert _source_codes(L, ctx.h, abi.ACCEPT_RESCORED) == (E, E, E)  # before a rescore
        assert b"rescore" in L.ecdna_ssa_last_error_message()
        pool = np.zeros((2, BINS), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_pool_accepted(ctx.h, 0, pool.ctypes.data) == E  # before an accept
        # the calls' own argument checks
        hists = np.ones((2, BINS), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_rescore(ctx.h, 0, hists.ctypes.data) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_rescore(ctx.h, 65, hists.ctypes.data) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_rescore(ctx.h, 2, None) == abi.E_INVALID
        hists[1] = 0
        assert L.ecdna_ssa_ctx_rescore(ctx.h, 2, hists.ctypes.data) == abi.E_INVALID
        assert b"target_hists[1]" in L.ecdna_ssa_last_error_message()
        rec = ctx.rescore(_targets())
        ctx.accept(abi.ACCEPT_RESCORED, [[INF] * 4])
        assert ctx.pool_accepted(0).sum() > 0
        assert L.ecdna_ssa_ctx_pool_accepted(ctx.h, 1, pool.ctypes.data) == abi.E_INVALID  # threshold >= Q
        assert L.ecdna_ssa_ctx_pool_accepted(ctx.h, 0, None) == abi.E_INVALID
        # a relaunch invalidates the records and the acceptance results
        ctx.launch()
        ctx.sync()
        out = np.zeros((P, 600), dtype=abi.STATS_DTYPE)
        assert L.ecdna_ssa_ctx_download_rescored(ctx.h, out.ctypes.data) == E
        assert L.ecdna_ssa_ctx_pool_accepted(ctx.h, 0, pool.ctypes.data) == E
        assert _source_codes(L, ctx.h, abi.ACCEPT_RESCORED) == (E, E, E)
        assert ctx.rescore(_targets()).tobytes() == rec.tobytes()  # ... and the same run gives the same records
    with engine_mod.Context(_keep_spec(store, kmax, None)) as ctx:
        assert ctx.keep is None and ctx.instance() == ins_on
        ctx.launch()
        ctx.sync()
        off = ctx.download(want_rows=True)
        assert _raw_calls(L, ctx.h, 600, 0) == (E, E, E, E)  # without the block
        assert b"ecdna_ssa_ctx_create_keep" in L.ecdna_ssa_last_error_message()
        assert _source_codes(L, ctx.h, abi.ACCEPT_RESCORED) == (E, E, E)
        assert _source_codes(L, ctx.h, 10) == (abi.E_INVALID,) * 3 == _source_codes(L, ctx.h, 11)
        with pytest.raises(engine_mod.EngineError, match="create_keep"):
            ctx.rescore(_targets())
    for name in ("summaries", "hist", "totals", "stats", "sample_stats", "sample_hist"):
        assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
    assert np.all(on.sample_stats["cells"] == np.minimum(on.summaries["nminus"] + on.summaries["nplus"], OWN_M))
    for i in range(600):
        np.testing.assert_array_equal(on.row(i), off.row(i))


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_limits(engine_mod, store, kmax):
    """The largest table beside the largest histogram, P = 64: 2,048 bins, m = 4096, 64 pure-birth replicates of 8,200
    cells (the spec of tests/test_gpu_cohort.py::test_limits). Targets 0 and 63 against their plain runs."""
    bins, n_targets, m = 2048, 64, 4096
    rng = np.random.default_rng(9)
    targets = rng.integers(0, 50, (n_targets, bins)).astype(np.uint64)
    targets[:, 0] += 1
    base = dict(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=bins, flags=_flags(store),
                bin_kmax=kmax)
    with _launched(engine_mod, abi.RunSpec(keep_cells=m, **base)) as ctx:
        summ = ctx.download().summaries
        assert np.all(summ["nminus"] + summ["nplus"] == 8200) and not (summ["error"] != 0).any()
        rec = ctx.rescore(targets)
        headers, _ = ctx.download_kept()
        assert np.all(headers["nminus"].astype(np.int64) + headers["nplus"] == m)
        ctx.accept(abi.ACCEPT_RESCORED, [[INF] * 4])
        pooled = ctx.pool_accepted(0)
    for p in (0, 63):
        plain = engine_mod.run(abi.RunSpec(stats_target=targets[p], subsample_cells=m, **base))
        assert rec[p].tobytes() == plain.sample_stats.tobytes(), p
        assert np.all(rec[p]["cells"] == m)
    np.testing.assert_array_equal(pooled, plain.sample_hist)
    assert pooled.sum() == 64 * m
