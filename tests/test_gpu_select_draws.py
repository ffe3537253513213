"""ABC thresholds over thinning draws (ecdna_ssa_ctx_select_draws and _select_draws_digits; thinned select mapping v1,
include/ecdna_ssa.h) on the GPU.

The mapping's contracts are equalities of integers or of bits. S1: every pass's digit array is the sum over the draws of
the digit arrays of the sized rescore's records at that draw — here formed in numpy from the downloaded records
(tests/select_draws_law.py) and compared element for element; S2: accept_draws with a found value as its one threshold
accepts exactly counts_le pairs; S3: one draw is ecdna_ssa_ctx_select after the sized rescore, bit for bit; S4: shards'
arrays sum and nothing depends on the placement."""
import ctypes as C

import numpy as np
import pytest

import select_draws_law as sdl
from ecdna_evo_amd import abi, shard
from support.draws_specs import FRACTIONS, KEEP, N, PER_SET, SIZES, TWO_STORES, _nk, _spec, _targets
from support.gpu import _bytes_of, _launched

INF = np.inf


def _mask(tp):
    return sum(1 << t for t in tp) if tp else 0


def _per_draw(ctx, store, targets, sizes, draws):
    """The records of the sized rescore at each draw, replicate-major [n][slots]: the loop the call replaces."""
    out = []
    for d in draws:
        rec = (ctx.rescore(targets, sizes, [d] * len(sizes)) if store == "keep"
               else ctx.rescore_timepoints(targets, sizes, d))
        out.append(np.ascontiguousarray(rec.T))
    return out


def _same(got, want, tag=""):
    assert got.population == want.population, tag
    np.testing.assert_array_equal(got.ranks, want.ranks, err_msg=f"{tag}: ranks")
    np.testing.assert_array_equal(got.values.view(np.uint64), want.values.view(np.uint64), err_msg=f"{tag}: values")
    np.testing.assert_array_equal(got.counts_le, want.counts_le, err_msg=f"{tag}: counts_le")


def _walked(digits, K, law_digits=None, tag="", **kw):
    """The walk over `digits(pass, prefixes)`; every pass's array against law_digits(pass, prefixes), element for
    element."""
    walk = shard.SelectWalk(K, **kw)
    for p in range(shard.SelectWalk.PASSES):
        got = digits(p, walk.prefixes)
        assert got.dtype == np.uint64 and got.shape == (4, K, 256)
        if law_digits is not None:
            np.testing.assert_array_equal(got, law_digits(p, walk.prefixes), err_msg=f"{tag}: pass {p}")
        walk.feed(got)
    return walk.result()


def _check_s1(ctx, store, targets, sizes, per, summ, first, nd, tp, tag, **kw):
    """S1 for one block and one set of ranks: the digit passes, the walk over them and select_draws against the law over
    the draws' records. Returns the result."""
    sub, mask = per[first:first + nd], _mask(tp)
    K = len(kw.get("ranks") or kw.get("fractions"))
    want = sdl.select(sub, summ, timepoint_mask=mask, **kw)
    tps = list(tp) if tp else None
    walked = _walked(lambda p, pre: ctx.select_draws_digits(targets, sizes, p, pre, nd, first, tps, store), K,
                     lambda p, pre: sdl.digit_hist(sub, summ, p, pre, mask), tag, **kw)
    _same(walked, want, tag + ": the walk")
    got = ctx.select_draws(targets, sizes, nd, first, tps, store, **kw)
    assert got.values.dtype == np.float64 and got.counts_le.dtype == np.uint64 and got.ranks.dtype == np.uint64
    _same(got, want, tag + ": select_draws")
    return got


# ---- 1 and 2. S1 exactly, and S2 on every finite value ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("bins", [9, 130])
def test_s1_equals_the_sum_over_the_draws_and_s2_cuts_where_accept_draws_cuts(engine_mod, store, kmax, bins):
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        summ = ctx.download().summaries
        nk = _nk(ctx.download_kept()[0])
        assert (nk == 0).sum() >= 3 and ((nk > 0) & (nk < 90)).sum() >= 10 and (nk == KEEP).sum() >= 100
        free = int((summ["error"] == 0).sum())
        per = _per_draw(ctx, "keep", t, SIZES, range(64))
        results = {}
        for tp in (None, (0, 2)):
            for first, nd in ((0, 64), (61, 3)):
                tag = f"timepoints {tp}, draws {first}..{first + nd - 1}"
                M = free * nd
                got = _check_s1(ctx, "keep", t, SIZES, per, summ, first, nd, tp, tag, fractions=FRACTIONS)
                assert got.population == M and got.ranks[-1] == M
                edge = _check_s1(ctx, "keep", t, SIZES, per, summ, first, nd, tp, tag, ranks=[1, M, M + 1])
                assert np.all(np.isinf(edge.values[:, 2])) and np.all(edge.counts_le[:, 2] == M)
                results[(tp, first, nd)] = got
        # the draws matter: the quantiles over 64 draws are not those over three
        assert _bytes_of(results[(None, 0, 64)])[2] != _bytes_of(results[(None, 61, 3)])[2]
        # S2: a found value as accept_draws' one threshold accepts exactly counts_le pairs; the next number below, fewer
        # than the rank
        for (tp, first, nd), got in results.items():
            tps = list(tp) if tp else None
            for x in range(4):
                for j in range(len(FRACTIONS)):
                    v = float(got.values[x, j])
                    if not np.isfinite(v):
                        continue
                    row = [INF] * 4
                    row[x] = v
                    acc = ctx.accept_draws(t, SIZES, [row], nd, first, tps)
                    assert int(acc.sums[0].sum()) == int(got.counts_le[x, j]) >= int(got.ranks[j]), (tp, first, x, j)
                    if v > 0.0:
                        row[x] = float(np.nextafter(v, -INF))
                        acc = ctx.accept_draws(t, SIZES, [row], nd, first, tps)
                        assert int(acc.sums[0].sum()) < int(got.ranks[j]), (tp, first, x, j)


# ---- 3. S3: one draw is the select on the rescored records ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_s3_one_draw_is_select_after_the_sized_rescore(engine_mod, store, kmax):
    bins = 33
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        for d in (0, 63):
            for tp in (None, [0, 2], [1]):
                ctx.rescore(t, SIZES, [d] * 3)
                want = ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS, timepoints=tp)
                got = ctx.select_draws(t, SIZES, 1, d, tp, fractions=FRACTIONS)
                assert _bytes_of(got) == _bytes_of(want), (d, tp)
                by_rank = [1, 7, want.population, want.population + 1]
                assert _bytes_of(ctx.select_draws(t, SIZES, 1, d, tp, ranks=by_rank)) == \
                    _bytes_of(ctx.select(abi.ACCEPT_RESCORED, ranks=by_rank, timepoints=tp)), (d, tp)
        assert want.population > 100 and len(np.unique(want.values[0])) >= 4


# ---- 4. the timepoint store ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_snapshot_timepoints(engine_mod, store, kmax):
    bins, m, sizes = 33, 50, (20, 50, 35, 28)
    t = _targets(bins, 4)
    spec = _spec(store, kmax, bins, keep_cells=None, snapshots=(10, 30, 100, 160), snapshot_stats=True,
                 keep_timepoint_cells=m)
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        taken = _nk(ctx.download_kept_timepoints()[0]) > 0
        assert taken[0].sum() >= 150 and not taken[3].all() and taken[3].any()  # untaken snapshots occur
        per = _per_draw(ctx, "timepoints", t, sizes, range(64))
        for tp in (None, (1, 3)):
            for first, nd in ((0, 64), (7, 2)):
                got = _check_s1(ctx, "timepoints", t, sizes, per, summ, first, nd, tp, f"timepoints {tp}, first {first}",
                                fractions=FRACTIONS)
                assert got.population == int((summ["error"] == 0).sum()) * nd
        # timepoint 1 alone is scored whole (30 cells at most, m1 = 50): its keys are one draw's, 64 times
        whole = ctx.select_draws(t, sizes, 64, 0, [1], "timepoints", fractions=FRACTIONS)
        one = ctx.select_draws(t, sizes, 1, 5, [1], "timepoints", fractions=FRACTIONS)
        assert whole.values.tobytes() == one.values.tobytes()
        np.testing.assert_array_equal(whole.counts_le, one.counts_le * np.uint64(64))


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_passage_timepoints(engine_mod, store, kmax):
    """Two growth phases passaged at 100 cells, 40 measured of each: the error rule per participating phase — a replicate
    extinct in phase 0 has its error in phase 1 only, and masking phase 1 out brings it back into the population."""
    bins, m, sizes, G, D = 33, 100, (40, 40), 2, 16
    t = _targets(bins, G)
    spec = _spec(store, kmax, bins, keep_cells=None, max_cells=500, max_time=None, init={0: 2, 1: 2, 12: 1},
                 cell_cap=1024, n_passages=G, passage_cells=m, passage_targets=t, keep_timepoint_cells=m)
    with _launched(engine_mod, spec) as ctx:
        psumm = ctx.download().passages.summaries  # [G][n]
        err = psumm["error"]
        only1 = (err[0] == 0) & (err[1] != 0)
        assert only1.any() and (err.sum(axis=0) == 0).sum() >= 100
        summ = np.ascontiguousarray(psumm.T)  # [n][G]: the rule per participating phase
        per = _per_draw(ctx, "timepoints", t, sizes, range(D))
        got = {tp: _check_s1(ctx, "timepoints", t, sizes, per, summ, 0, D, tp, f"phases {tp}", fractions=FRACTIONS)
               for tp in (None, (0,), (1,))}
        assert got[None].population == int((err.sum(axis=0) == 0).sum()) * D
        assert got[(0,)].population - got[None].population == int(only1.sum()) * D > 0


# ---- 5. whole samples, errors, empty samples, guard headers ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_whole_samples_errors_and_empty_samples(engine_mod, store, kmax):
    bins, nd, first = 9, 10, 3
    t = _targets(bins)
    zeros = np.zeros((4, 1), dtype=np.uint64)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        summ = ctx.download().summaries
        nk = _nk(ctx.download_kept()[0])
        bad, free = summ["error"] != 0, summ["error"] == 0
        assert ((nk == 0) & free).sum() >= 3 and ((nk <= 90) & free).sum() >= 10
        # pass 0 counts every key, (error-free) x D of them
        hist = ctx.select_draws_digits(t, SIZES, 0, zeros, nd, first)
        assert np.all(hist.sum(axis=2) == int(free.sum()) * nd)
        # the empty kept samples {0, 0}: ks = 1.0 exactly on every draw, and no ks is larger: the top (empty) x D keys
        M, empty = int(free.sum()) * nd, int(((nk == 0) & free).sum()) * nd
        top = ctx.select_draws(t, SIZES, nd, first, ranks=[M - empty + 1, M])
        assert np.all(top.values[0] == 1.0) and np.all(top.counts_le[0] == M)
        # a size >= every a + b: every replicate is scored whole, all D keys of a replicate are equal — the keys of the
        # one rescore at that size, D times each
        full = (KEEP,) * 3
        ctx.rescore(t, full, [0] * 3)
        ranks = [1, 2, 17, 100, int(free.sum())]
        one = ctx.select(abi.ACCEPT_RESCORED, ranks=ranks)
        for k_of in (lambda k: (k - 1) * nd + 1, lambda k: k * nd):  # the first and the last of a key's D copies
            many = ctx.select_draws(t, full, nd, first, ranks=[k_of(k) for k in ranks])
            assert many.population == one.population * nd
            assert many.values.tobytes() == one.values.tobytes()
            np.testing.assert_array_equal(many.counts_le, one.counts_le * np.uint64(nd))
        # ... and the replicates below 90 cells are whole at SIZES too: the per-draw law says the same
        per = _per_draw(ctx, "keep", t, SIZES, range(first, first + nd))
        small = (nk <= 90) & free
        for f in ("ks", "mean_rel", "entropy_rel", "frequency_diff"):
            assert all(np.array_equal(r[f][small], per[0][f][small]) for r in per)
        want = sdl.select(per, summ, fractions=FRACTIONS)
        _same(ctx.select_draws(t, SIZES, nd, first, fractions=FRACTIONS), want, "the law")


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_error_replicates_are_in_no_histogram_row(engine_mod, store, kmax):
    """The middle set starts from an empty population: its 86 replicates end with ECDNA_REP_ERR_EMPTY and are in no
    draw's keys."""
    bins, nd, first = 9, 5, 59
    t = _targets(bins)
    start = {0: 1, 1: 1, 12: 1}
    with _launched(engine_mod, _spec(store, kmax, bins, init=None, init_per_set=[start, {}, start])) as ctx:
        summ = ctx.download().summaries
        bad = summ["error"] != 0
        assert bad.sum() >= 1 and np.all(summ["error"][PER_SET:2 * PER_SET] == abi.REP_ERR_EMPTY)
        free = int((~bad).sum())
        hist = ctx.select_draws_digits(t, SIZES, 0, np.zeros((4, 1), dtype=np.uint64), nd, first)
        assert np.all(hist.sum(axis=2) == free * nd)
        per = _per_draw(ctx, "keep", t, SIZES, range(64))
        for tp in (None, (1,)):
            got = _check_s1(ctx, "keep", t, SIZES, per, summ, first, nd, tp, f"timepoints {tp}", ranks=[1, free * nd, N * nd])
            assert got.population == free * nd and np.all(np.isinf(got.values[:, 2]))


@pytest.mark.gpu
def test_guard_headers_contribute_the_key_of_zero(engine_mod):
    """The state of tests/test_gpu_sample_states.py::test_end_to_end_at_the_size_guard: every kept header is the
    guard's, every record all zero — every key is key(0.0)."""
    from support.state_specs import E2E_BINS, _e2e_spec

    spec = _e2e_spec("bins", {0: 2**32 - 3, 1: 2}, max_cells=10, cell_cap=64)
    t = _targets(E2E_BINS, 2)
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        free = int((summ["error"] == 0).sum())
        headers, _ = ctx.download_kept()
        assert np.all(headers["nminus"] == abi.KEPT_GUARD) and np.all(headers["nplus"] == abi.KEPT_GUARD)
        per = _per_draw(ctx, "keep", t, (200, 1), (62, 63))
        assert free >= 1 and all(not r[f].any() for r in per for f in ("ks", "mean_rel", "entropy_rel", "frequency_diff"))
        got = _check_s1(ctx, "keep", t, (200, 1), per, summ, 0, 2, None, "guards", ranks=[1, 2 * free, 2 * free + 1])
        # (per holds draws 62 and 63 at entries 0 and 1; a guard's records do not depend on the draw)
        assert _bytes_of(ctx.select_draws(t, (200, 1), 2, 62, ranks=[1, 2 * free, 2 * free + 1])) == _bytes_of(got)
        assert got.population == 2 * free
        assert np.all(got.values[:, :2].view(np.uint64) == 0) and np.all(got.counts_le == 2 * free)
        hist = ctx.select_draws_digits(t, (200, 1), 0, np.zeros((4, 1), dtype=np.uint64), 2, 62)
        assert np.all(hist[:, 0, 0x80] == 2 * free) and hist.sum() == 4 * 2 * free  # key(0.0) = 0x8000000000000000


# ---- 6. shards and placement ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_shards_sum_and_the_placement_does_not_matter(engine_mod, store, kmax, monkeypatch, tmp_path):
    import torch.distributed as dist

    bins, nd, first = 33, 24, 5
    t = _targets(bins)
    K = len(FRACTIONS)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        whole = ctx.select_draws(t, SIZES, nd, first, fractions=FRACTIONS)
        digits = []
        _walked(lambda p, pre: digits.append(ctx.select_draws_digits(t, SIZES, p, pre, nd, first)) or digits[-1], K,
                fractions=FRACTIONS)
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            sharded = shard.select_draws(ctx, t, SIZES, nd, first, fractions=FRACTIONS)
            masked = shard.select_draws(ctx, t, SIZES, 3, 61, timepoints=(0, 2), ranks=[1, 50])
        finally:
            dist.destroy_process_group()
        assert _bytes_of(sharded) == _bytes_of(whole)
        assert _bytes_of(masked) == _bytes_of(ctx.select_draws(t, SIZES, 3, 61, [0, 2], ranks=[1, 50]))
    assert len(np.unique(whole.values[0])) >= 4 and whole.population > 100 * nd
    # two interleaved shard contexts, each with its own keys: their digit arrays, summed per pass, are the whole run's
    parts = [_launched(engine_mod, _spec(store, kmax, bins, first_replicate=g, replicate_stride=2,
                                         n_replicates=len(range(g, N, 2)))) for g in range(2)]
    try:
        passes = []

        def summed(p, pre):
            passes.append(sum(part.select_draws_digits(t, SIZES, p, pre, nd, first) for part in parts))
            return passes[-1]

        _same(_walked(summed, K, fractions=FRACTIONS), whole, "two shards")
        for p in range(8):
            np.testing.assert_array_equal(passes[p], digits[p], err_msg=f"pass {p}")
    finally:
        for part in parts:
            part.close()
    # forced chunks, and a capped stepper grid
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_spec(store, kmax, bins)) as ctx:
        assert ctx.instance()["n_chunks"] == 3
        ctx.launch()
        ctx.sync()
        assert _bytes_of(ctx.select_draws(t, SIZES, nd, first, fractions=FRACTIONS)) == _bytes_of(whole)
    monkeypatch.delenv("ECDNA_SSA_MAX_CHUNK")
    monkeypatch.setenv("ECDNA_SSA_MAX_BLOCKS", "2")
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        assert _bytes_of(ctx.select_draws(t, SIZES, nd, first, fractions=FRACTIONS)) == _bytes_of(whole)


# ---- 7. nothing else moves ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_nothing_else_moves(engine_mod, store, kmax):
    bins = 33
    t = _targets(bins)
    L = engine_mod.lib()
    zeros = np.zeros((4, 2), dtype=np.uint64)

    def state(ctx):
        acc = ctx.download_accept()
        adr = ctx.download_accept_draws()
        sel = ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))
        return (ctx.download_rescored().tobytes(), acc.counts.tobytes(), acc.mask.tobytes(), acc.n_accepted,
                acc.ids.tobytes(), acc.stats.tobytes(), sel.population, sel.values.tobytes(), sel.counts_le.tobytes(),
                ctx.pool_accepted(1).tobytes(), adr.passes.tobytes(), adr.sums.tobytes())

    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        # the call works before any rescore, and leaves the store without records
        first = ctx.select_draws(t, SIZES, 8, fractions=FRACTIONS)
        assert first.population > 100 * 8 and len(np.unique(first.values[0])) >= 4
        assert L.ecdna_ssa_ctx_download_rescored(ctx.h, None) == abi.E_STATE
        thr = [[0.5, INF, INF, INF], [INF, 0.3, INF, 0.2], [INF] * 4]
        ctx.rescore(t, (199, 60, 130), (1, 2, 3))
        ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))  # (leaves cached keys)
        ctx.accept(abi.ACCEPT_RESCORED, thr, None, 1, 50)
        ctx.accept_draws(t, SIZES, thr, 8)
        before = state(ctx)
        again = ctx.select_draws(t, SIZES, 8, fractions=FRACTIONS)
        assert _bytes_of(again) == _bytes_of(first)
        ctx.select_draws(t[:1], (77,), 64, 0, ranks=[5])  # (other sizes of every buffer)
        for p in range(3):
            ctx.select_draws_digits(t, SIZES, p, zeros, 8)
        assert state(ctx) == before
        # the keys are one block's: a pass above 0 reads them only for the block pass 0 made them for
        walk = shard.SelectWalk(2, fractions=(0.5, 1.0))
        walk.feed(ctx.select_draws_digits(t, SIZES, 0, walk.prefixes, 8))
        pre = walk.prefixes  # (pass 1's: the top bytes of the median and of the largest key of each distance)
        h1 = ctx.select_draws_digits(t, SIZES, 1, pre, 8)
        assert h1.sum() > 0
        for changed in (dict(sample_cells=(90, 131, 90)), dict(n_draws=7), dict(first_draw=1), dict(timepoints=[0, 2])):
            kw = dict(sample_cells=SIZES, n_draws=8, first_draw=0, timepoints=None)
            kw.update(changed)
            with pytest.raises(engine_mod.EngineError, match="pass 0 of the same block must come first"):
                ctx.select_draws_digits(t, kw["sample_cells"], 1, pre, kw["n_draws"], kw["first_draw"], kw["timepoints"])
        t2 = t.copy()
        t2[1, 3] += 1
        with pytest.raises(engine_mod.EngineError, match="pass 0 of the same block must come first"):
            ctx.select_draws_digits(t2, SIZES, 1, pre, 8)
        np.testing.assert_array_equal(ctx.select_draws_digits(t, SIZES, 1, pre, 8), h1)  # (the keys are still there)
        assert state(ctx) == before
        # a relaunch drops the keys
        ctx.launch()
        ctx.sync()
        blk, _alive = ctx._accept_draws_block(t, SIZES, None, 8, 0, None, "keep")
        out = np.zeros((4, 2, 256), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_select_draws_digits(ctx.h, C.byref(blk), 1, 2, pre.ctypes.data,
                                                   out.ctypes.data) == abi.E_STATE
        assert b"pass 0 of the same block must come first" in L.ecdna_ssa_last_error_message()
        ctx.select_draws_digits(t, SIZES, 0, pre, 8)  # pass 0 afterwards works again
        np.testing.assert_array_equal(ctx.select_draws_digits(t, SIZES, 1, pre, 8), h1)
        assert _bytes_of(ctx.select_draws(t, SIZES, 8, fractions=FRACTIONS)) == _bytes_of(first)


@pytest.mark.gpu
def test_the_timepoint_stores_records_do_not_move(engine_mod):
    bins, m, sizes = 33, 50, (20, 50, 35)
    t = _targets(bins)
    spec = _spec("bins", 64, bins, keep_cells=None, snapshots=(10, 30, 100), snapshot_stats=True, keep_timepoint_cells=m)
    with _launched(engine_mod, spec) as ctx:
        ctx.rescore_timepoints(t, sizes, 4)
        sel = ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=(0.5,))
        before = (ctx.download_rescored_timepoints().tobytes(), sel.values.tobytes(), sel.counts_le.tobytes())
        got = ctx.select_draws(t, sizes, 64, 0, None, "timepoints", fractions=FRACTIONS)
        assert got.population == sel.population * 64
        sel = ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=(0.5,))
        assert (ctx.download_rescored_timepoints().tobytes(), sel.values.tobytes(), sel.counts_le.tobytes()) == before


# ---- 8. refusals ----

def _block(hists, cells, **kw):
    cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.uint32)
    a = abi.AcceptDraws(struct_size=C.sizeof(abi.AcceptDraws), n_targets=hists.shape[0], n_draws=64)
    a.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    if cells is not None:
        a.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
    for k, v in kw.items():
        setattr(a, k, v)
    return a, (hists, cells)


@pytest.mark.gpu
def test_refusals(engine_mod):
    L = engine_mod.lib()
    bins, m = 9, 20
    hists = np.ones((65, bins), dtype=np.uint64)
    two = np.ascontiguousarray(hists[:2])
    base = dict(n_replicates=4, max_cells=50, hist_bins=bins, flags=abi.FLAG_REP_STATS)
    half = np.asarray([0.5, 1.0])
    rk = np.asarray([1, 2], dtype=np.uint64)
    pre = np.zeros((4, 2), dtype=np.uint64)
    out = np.zeros((4, 2, 256), dtype=np.uint64)
    thr = np.full((1, 4), INF)

    def call(ctx, *a, ranks=None, fractions=half, K=2, **kw):
        blk, keep = _block(*a, **kw)
        rc = L.ecdna_ssa_ctx_select_draws(ctx.h, C.byref(blk), K, None if ranks is None else ranks.ctypes.data,
                                          None if fractions is None else fractions.ctypes.data, None, None, None, None)
        return rc, L.ecdna_ssa_last_error_message().decode()

    def digits(ctx, *a, pass_=0, K=2, prefixes=pre, out_hist=out, **kw):
        blk, keep = _block(*a, **kw)
        rc = L.ecdna_ssa_ctx_select_draws_digits(ctx.h, C.byref(blk), pass_, K,
                                                 None if prefixes is None else prefixes.ctypes.data,
                                                 None if out_hist is None else out_hist.ctypes.data)
        return rc, L.ecdna_ssa_last_error_message().decode()

    def refused(ctx, word, *a, **kw):
        for f in (call, digits):
            rc, msg = f(ctx, *a, **kw)
            assert rc == abi.E_INVALID and word in msg, (word, rc, msg)

    with engine_mod.Context(abi.RunSpec(keep_cells=m, **base)) as ctx:
        refused(ctx, "sample_cells[1]", two, (5, m + 1))  # a bad block is refused before the state is looked at
        assert call(ctx, two, (5, m))[0] == abi.E_STATE and digits(ctx, two, (5, m))[0] == abi.E_STATE  # before a launch
        ctx.launch()
        ctx.sync()
        assert L.ecdna_ssa_ctx_select_draws(ctx.h, None, 2, None, half.ctypes.data, None, None, None,
                                            None) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_select_draws_digits(ctx.h, None, 0, 2, pre.ctypes.data, out.ctypes.data) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_select_draws(None, None, 2, None, half.ctypes.data, None, None, None,
                                            None) == abi.E_INVALID
        # the call finds the thresholds: a block that brings some is refused
        refused(ctx, "select_draws.n_thresholds", two, (5, 5), n_thresholds=1,
                thresholds=thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold)))
        refused(ctx, "select_draws.n_thresholds", two, (5, 5), n_thresholds=1)
        refused(ctx, "select_draws.thresholds", two, (5, 5), thresholds=thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold)))
        # everything else accept_draws refuses, with its messages
        refused(ctx, "accept_draws.struct_size", two, (5, 5), struct_size=C.sizeof(abi.AcceptDraws) + 8)
        refused(ctx, "accept_draws.reserved", two, (5, 5), reserved=1)
        refused(ctx, "accept_draws.timepoints", two, (5, 5), timepoints=2)
        refused(ctx, "accept_draws.n_targets", two, (5, 5), n_targets=0)
        refused(ctx, "accept_draws.n_targets", hists, (5,) * 65)
        blk, keep = _block(two, (5, 5))
        blk.target_hists = None
        assert L.ecdna_ssa_ctx_select_draws(ctx.h, C.byref(blk), 2, None, half.ctypes.data, None, None, None,
                                            None) == abi.E_INVALID
        assert b"target_hists is NULL" in L.ecdna_ssa_last_error_message()
        holed = two.copy()
        holed[1] = 0
        refused(ctx, "target_hists[1]", holed, (5, 5))
        refused(ctx, "sample_cells is NULL", two, None)
        refused(ctx, "sample_cells[0]", two, (0, 5))
        refused(ctx, "keep_cells = 20", two, (5, m + 1))
        refused(ctx, "accept_draws.n_draws", two, (5, 5), n_draws=0)
        refused(ctx, "accept_draws.n_draws", two, (5, 5), n_draws=65)
        refused(ctx, "first_draw", two, (5, 5), first_draw=1)  # 1 + 64 > 64
        refused(ctx, "first_draw", two, (5, 5), first_draw=64, n_draws=1)
        refused(ctx, "timepoint_mask", two, (5, 5), timepoint_mask=0b100)
        # the rank rules of ecdna_ssa_select_t
        for K in (0, 33):
            rc, msg = call(ctx, two, (5, 5), K=K)
            assert rc == abi.E_INVALID and "select_draws.n_ranks" in msg
        rc, msg = call(ctx, two, (5, 5), ranks=rk)  # both
        assert rc == abi.E_INVALID and "exactly one of select_draws.ranks and select_draws.fractions" in msg
        rc, msg = call(ctx, two, (5, 5), fractions=None)  # neither
        assert rc == abi.E_INVALID and "exactly one of select_draws.ranks and select_draws.fractions" in msg
        rc, msg = call(ctx, two, (5, 5), ranks=np.asarray([3, 0], dtype=np.uint64), fractions=None)
        assert rc == abi.E_INVALID and "select_draws.ranks[1]" in msg
        for f in (0.0, 1.5, np.nan):
            rc, msg = call(ctx, two, (5, 5), fractions=np.asarray([0.5, f]))
            assert rc == abi.E_INVALID and "select_draws.fractions[1]" in msg
        # the rules of a digit pass
        rc, msg = digits(ctx, two, (5, 5), pass_=8)
        assert rc == abi.E_INVALID and "select_draws_digits.pass" in msg
        for K in (0, 33):
            rc, msg = digits(ctx, two, (5, 5), K=K)
            assert rc == abi.E_INVALID and "select_draws_digits.n_prefixes" in msg
        rc, msg = digits(ctx, two, (5, 5), prefixes=None)
        assert rc == abi.E_INVALID and "select_draws_digits.prefixes is NULL" in msg
        rc, msg = digits(ctx, two, (5, 5), out_hist=None)
        assert rc == abi.E_INVALID and "select_draws_digits.out_hist is NULL" in msg
        # states
        rc, msg = call(ctx, two, (5, 5), timepoints=1)  # a keep context has no timepoint block
        assert rc == abi.E_STATE and "create_keep_timepoints" in msg
        rc, msg = digits(ctx, two, (5, 5), pass_=3)  # no pass 0 yet
        assert rc == abi.E_STATE and "pass 0 of the same block must come first" in msg
        with pytest.raises(engine_mod.EngineError, match="sample_cells"):
            ctx.select_draws(two, (5, m + 1), fractions=(0.5,))
        with pytest.raises(ValueError):
            ctx.select_draws(two, (5, 5), store="snapshots", fractions=(0.5,))
        with pytest.raises(ValueError):
            ctx.select_draws(two, (5, 5))
        # ... and the context stays usable: a good block is taken
        assert call(ctx, two, (5, m), first_draw=63, n_draws=1, timepoint_mask=0b10)[0] == abi.OK
        got = ctx.select_draws(two, (5, m), fractions=(0.5, 1.0))
        free = int((ctx.download().summaries["error"] == 0).sum())
        assert got.population == free * 64 and got.values.shape == (4, 2) and got.ranks[1] == free * 64
        assert digits(ctx, two, (5, m))[0] == abi.OK and digits(ctx, two, (5, m), pass_=7)[0] == abi.OK
    with engine_mod.Context(abi.RunSpec(**base)) as ctx:  # a context without either block
        ctx.launch()
        ctx.sync()
        rc, msg = call(ctx, two, (5, 5))
        assert rc == abi.E_STATE and "ecdna_ssa_ctx_create_keep" in msg
        assert digits(ctx, two, (5, 5), timepoints=1)[0] == abi.E_STATE
    spec = abi.RunSpec(snapshots=(10, 30), snapshot_stats=True, keep_timepoint_cells=m, **base)
    with engine_mod.Context(spec) as ctx:
        three = np.ascontiguousarray(hists[:3])
        refused(ctx, "n_targets must be T = 2", three, (5, 5, 5), timepoints=1)
        assert call(ctx, two, (5, m), timepoints=1)[0] == abi.E_STATE  # before a launch
        rc, msg = call(ctx, two, (5, m))  # ... and it has no keep block
        assert rc == abi.E_STATE and "ecdna_ssa_ctx_create_keep" in msg
        ctx.launch()
        ctx.sync()
        refused(ctx, "timepoint_mask", two, (5, m), timepoints=1, timepoint_mask=0b100)
        assert call(ctx, two, (5, m), timepoints=1, timepoint_mask=0b10)[0] == abi.OK
        assert ctx.select_draws(two, (5, m), 3, 61, store="timepoints", ranks=[1]).values.shape == (4, 1)
