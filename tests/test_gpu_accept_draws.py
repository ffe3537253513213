"""Acceptance over repeated thinnings of the kept samples (ecdna_ssa_accept_draws_t, ecdna_ssa_ctx_accept_draws and
_download_accept_draws; thinned acceptance mapping v1, include/ecdna_ssa.h).

The mapping's contract is an equality: passes[i][q] is the sum over the draws d of bit q of the mask that the sized
rescore at draw d followed by the acceptance pass gives. Most tests here run that loop and compare integers, element for
element; one compares with the numpy restatement (tests/accept_draws_law.py) at thresholds that lie in gaps of the law's
own distances, so that the float tolerance of the records cannot flip a verdict."""
import ctypes as C

import numpy as np
import pytest

import accept_draws_law as adl
import accept_law as al
from ecdna_evo_amd import abi
from support.draws_specs import (FRACTIONS, KEEP, N, PER_SET, SEED, SETS, SIZES, TWO_STORES, _block, _gap_thresholds,
                                 _nk, _rows, _spec, _targets)
from support.gpu import _flags, _launched

INF = np.inf


def _bits(mask, Q):
    return ((mask[:, None] >> np.arange(Q, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.uint8)


def _loop(ctx, store, targets, sizes, thr, draws, timepoint_sets):
    """The loop the call replaces: per draw, the sized rescore and one accept per set of timepoints. {timepoints:
    (bits [D][n][Q] u8, counts [D][Q][sets] u64)}."""
    Q = len(thr)
    out = {tp: ([], []) for tp in timepoint_sets}
    for d in draws:
        if store == "keep":
            ctx.rescore(targets, sizes, [d] * len(sizes))
            source = abi.ACCEPT_RESCORED
        else:
            ctx.rescore_timepoints(targets, sizes, d)
            source = abi.ACCEPT_RESCORED_TIMEPOINTS
        for tp in timepoint_sets:
            r = ctx.accept(source, thr, list(tp) if tp else None)
            out[tp][0].append(_bits(r.mask, Q))
            out[tp][1].append(r.counts.copy())
    return {tp: (np.asarray(b), np.asarray(c)) for tp, (b, c) in out.items()}


def _same(got, bits, counts, ids, per_set, tag):
    """An AcceptDrawsResult against the loop's bits and counts of the same draws."""
    want = bits.sum(axis=0).astype(np.uint8)
    assert got.passes.dtype == np.uint8 and got.passes.shape == want.shape and got.sums.dtype == np.uint64
    np.testing.assert_array_equal(got.passes, want, err_msg=f"{tag}: passes")
    np.testing.assert_array_equal(got.sums, counts.sum(axis=0), err_msg=f"{tag}: sums against the accepts' counts")
    sets = (np.asarray(ids, dtype=np.uint64) // np.uint64(per_set)).astype(np.int64)
    for q in range(want.shape[1]):
        by_set = np.bincount(sets, weights=got.passes[:, q], minlength=got.sums.shape[1]).astype(np.uint64)
        np.testing.assert_array_equal(got.sums[q], by_set, err_msg=f"{tag}: sums of row {q} against passes")


# ---- 1. equals the composition, exactly ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("bins", [9, 130])
def test_equals_the_loop_of_rescore_and_accept(engine_mod, store, kmax, bins):
    t = _targets(bins)
    spec = _spec(store, kmax, bins)
    tps = (None, (0, 2))
    with _launched(engine_mod, spec) as ctx:
        headers, _ = ctx.download_kept()
        nk = _nk(headers)
        assert (nk == 0).sum() >= 3 and ((nk > 0) & (nk < 90)).sum() >= 10 and (nk == KEEP).sum() >= 100
        ctx.rescore(t, SIZES, [0] * 3)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        loop = _loop(ctx, "keep", t, SIZES, thr, range(64), tps)
        for tp in tps:
            bits, counts = loop[tp]
            for first, nd in ((0, 64), (61, 3)):
                got = ctx.accept_draws(t, SIZES, thr, nd, first, list(tp) if tp else None)
                assert got.n_draws == nd
                _same(got, bits[first:first + nd], counts[first:first + nd], spec.replicate_ids(), PER_SET,
                      f"timepoints {tp}, draws {first}..{first + nd - 1}")
                if nd == 64:  # the thresholds decide, and differently from draw to draw
                    assert ((got.passes > 0) & (got.passes < 64)).any(axis=0).sum() >= 3
                    assert got.passes[:, 31].max() == 64
        assert (loop[None][0].sum(axis=0) != loop[(0, 2)][0].sum(axis=0)).any()  # target 1 decides for somebody


# ---- 2. equals the restatement ----


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_equals_the_restatement(engine_mod, store, kmax):
    bins, first, nd = 9, 2, 4
    t = _targets(bins)
    spec = _spec(store, kmax, bins)
    ids = spec.replicate_ids()
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        headers, cells = ctx.download_kept()
        slots = [adl.Slot(headers, cells, t[p], SIZES[p], SEED) for p in range(3)]
        per_draw = [adl.records(slots, ids, bins, d) for d in range(first, first + nd)]
        free = summ["error"] == 0
        picks = (0.1, 0.35, 0.6, 0.9)
        cuts = [_gap_thresholds(np.concatenate([r[f][free].ravel() for r in per_draw]), picks) for f in al.FIELDS]
        thr = [[cuts[x][(q + x) % 4] if (q >> x) & 1 else INF for x in range(4)] for q in range(16)]
        for tp in (None, [1], [0, 2]):
            mask = sum(1 << p for p in tp) if tp else 0
            want_p, want_s = adl.accept_draws(slots, summ, ids, bins, PER_SET, SETS, thr, first, nd, mask, per_draw)
            got = ctx.accept_draws(t, SIZES, thr, nd, first, tp)
            np.testing.assert_array_equal(got.passes, want_p, err_msg=f"timepoints {tp}")
            np.testing.assert_array_equal(got.sums, want_s, err_msg=f"timepoints {tp}")
            assert ((want_p > 0) & (want_p < nd)).any()


# ---- 3. snapshots ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_snapshot_timepoints(engine_mod, store, kmax):
    bins, m, sizes = 33, 50, (20, 50, 35)
    t = _targets(bins)
    spec = _spec(store, kmax, bins, keep_cells=None, snapshots=(10, 30, 100), snapshot_stats=True,
                 keep_timepoint_cells=m)
    tps = (None, (0,), (1,), (2,), (0, 2))
    with _launched(engine_mod, spec) as ctx:
        headers, _ = ctx.download_kept_timepoints()
        taken = _nk(headers) > 0
        assert taken[0].sum() >= 150 and not taken[2].all() and taken[2].sum() >= 30  # untaken snapshots occur
        ctx.rescore_timepoints(t, sizes, 0)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=FRACTIONS).values)
        loop = _loop(ctx, "timepoints", t, sizes, thr, range(64), tps)
        for tp in tps:
            bits, counts = loop[tp]
            for first, nd in ((0, 64), (7, 2)):
                got = ctx.accept_draws(t, sizes, thr, nd, first, list(tp) if tp else None, store="timepoints")
                _same(got, bits[first:first + nd], counts[first:first + nd], spec.replicate_ids(), PER_SET,
                      f"timepoints {tp}, draws {first}..{first + nd - 1}")
        # timepoints 0 and 1 are scored whole (10 and 30 cells, below their m1 = 20 and 50): the same verdict on every
        # draw; timepoint 2 (35 of 50 kept cells) varies with the draw, and so does the joint verdict
        for tp in ((0,), (1,)):
            assert np.all(np.isin(loop[tp][0].sum(axis=0), (0, 64))), tp
        assert ((loop[(2,)][0].sum(axis=0) % 64) != 0).any() and ((loop[None][0].sum(axis=0) % 64) != 0).any()


# ---- 4. passages ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_passage_timepoints(engine_mod, store, kmax):
    """Two growth phases passaged at 100 cells, 40 measured of each: every phase under its own key, and the error rule
    per participating phase — a replicate extinct in phase 0 has its error in phase 1 only, and masking phase 1 out
    re-admits it."""
    bins, m, sizes, G = 33, 100, (40, 40), 2
    t = _targets(bins, G)
    spec = _spec(store, kmax, bins, keep_cells=None, max_cells=500, max_time=None, init={0: 2, 1: 2, 12: 1},
                 cell_cap=1024, n_passages=G, passage_cells=m, passage_targets=t, keep_timepoint_cells=m)
    tps = (None, (0,), (1,))
    with _launched(engine_mod, spec) as ctx:
        err = ctx.download().passages.summaries["error"]  # [G][n]
        only1 = (err[0] == 0) & (err[1] != 0)
        assert only1.any() and (err.sum(axis=0) == 0).sum() >= 100
        ctx.rescore_timepoints(t, sizes, 0)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=FRACTIONS).values, Q=12)
        loop = _loop(ctx, "timepoints", t, sizes, thr, range(16), tps)
        got = {}
        for tp in tps:
            got[tp] = ctx.accept_draws(t, sizes, thr, 16, 0, list(tp) if tp else None, store="timepoints")
            _same(got[tp], *loop[tp], spec.replicate_ids(), PER_SET, f"timepoints {tp}")
        # the all-inf row: the error rule alone
        assert np.all(got[None].passes[only1] == 0) and np.all(got[(1,)].passes[only1] == 0)
        assert np.all(got[(0,)].passes[only1, 11] == 16)
        assert np.all(got[None].passes[err.sum(axis=0) == 0, 11] == 16)


# ---- 5. placement ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_placement_independence(engine_mod, store, kmax, monkeypatch):
    """Forced chunks and three interleaved shards give the whole run's passes by global id, and sums that add up."""
    bins = 33
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        ctx.rescore(t, SIZES, [0] * 3)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        whole = ctx.accept_draws(t, SIZES, thr, 24, 5)
    assert ((whole.passes > 0) & (whole.passes < 24)).any() and whole.sums.sum() > 0
    total = np.zeros_like(whole.sums)
    for g in range(3):
        n = len(range(g, N, 3))
        with _launched(engine_mod, _spec(store, kmax, bins, first_replicate=g, replicate_stride=3,
                                         n_replicates=n)) as part:
            got = part.accept_draws(t, SIZES, thr, 24, 5)
        np.testing.assert_array_equal(got.passes, whole.passes[g::3], err_msg=f"shard {g}")
        total += got.sums
    np.testing.assert_array_equal(total, whole.sums)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_spec(store, kmax, bins)) as ctx:
        assert ctx.instance()["n_chunks"] == 3
        ctx.launch()
        ctx.sync()
        got = ctx.accept_draws(t, SIZES, thr, 24, 5)
    assert got.passes.tobytes() == whole.passes.tobytes() and got.sums.tobytes() == whole.sums.tobytes()


# ---- 6. nothing else moves ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_nothing_else_moves(engine_mod, store, kmax):
    bins = 33
    t = _targets(bins)
    L = engine_mod.lib()

    def state(ctx):
        acc = ctx.download_accept()
        sel = ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))
        return (ctx.download_rescored().tobytes(), acc.counts.tobytes(), acc.mask.tobytes(), acc.n_accepted,
                acc.ids.tobytes(), acc.stats.tobytes(), sel.population, sel.values.tobytes(), sel.counts_le.tobytes(),
                ctx.pool_accepted(1).tobytes())

    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        # the call works before any rescore, and leaves the store without records
        thr = [[0.5, INF, INF, INF], [INF, 0.3, INF, 0.2], [INF] * 4]
        first = ctx.accept_draws(t, SIZES, thr, 8)
        assert first.passes.shape == (N, 3) and first.sums.shape == (3, SETS) and first.passes[:, 2].max() == 8
        assert L.ecdna_ssa_ctx_download_rescored(ctx.h, None) == abi.E_STATE
        with pytest.raises(engine_mod.EngineError):
            ctx.accept(abi.ACCEPT_RESCORED, thr)
        ctx.rescore(t, (199, 60, 130), (1, 2, 3))
        ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))  # (leaves cached keys)
        ctx.accept(abi.ACCEPT_RESCORED, thr, None, 1, 50)
        before = state(ctx)
        again = ctx.accept_draws(t, SIZES, thr, 8)
        assert again.passes.tobytes() == first.passes.tobytes() and again.sums.tobytes() == first.sums.tobytes()
        ctx.accept_draws(t[:1], (77,), _rows(np.full((4, 2), 0.25)), 64, 0)  # (other sizes of every buffer)
        assert state(ctx) == before
        assert ctx.download_accept_draws().passes.shape == (N, 32)
        # a relaunch invalidates the results
        ctx.launch()
        ctx.sync()
        assert L.ecdna_ssa_ctx_download_accept_draws(ctx.h, None, None) == abi.E_STATE
        assert b"accept_draws" in L.ecdna_ssa_last_error_message()
        back = ctx.accept_draws(t, SIZES, thr, 8)
        assert back.passes.tobytes() == first.passes.tobytes()


# ---- 7. limits ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_limits(engine_mod, store, kmax):
    """The largest table (m' = 2048 of 4,096 kept cells) beside the largest histogram (2,048 bins): nothing is refused at
    launch and the counts are the loop's; and the smallest call, one row and one draw."""
    bins, m, sizes = 2048, 4096, (2048,)
    rng = np.random.default_rng(9)
    t = rng.integers(0, 50, (1, bins)).astype(np.uint64)
    t[:, 0] += 1
    spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=bins,
                       flags=_flags(store), bin_kmax=kmax, keep_cells=m)
    with _launched(engine_mod, spec) as ctx:
        headers, _ = ctx.download_kept()
        assert np.all(_nk(headers) == m)
        ctx.rescore(t, sizes, [0])
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        loop = _loop(ctx, "keep", t, sizes, thr, (62, 63), (None,))[None]
        _same(ctx.accept_draws(t, sizes, thr, 2, 62), *loop, spec.replicate_ids(), 64, "2,048 bins, m' = 2048")
        one = ctx.accept_draws(t, sizes, thr[3:4], 1, 63)
        assert one.passes.shape == (64, 1) and one.sums.shape == (1, 1)
        np.testing.assert_array_equal(one.passes[:, 0], loop[0][1][:, 3])
        assert one.sums[0, 0] == loop[1][1][3, 0]


# ---- 8. whole samples and guards ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_whole_samples_errors_and_empty_samples(engine_mod, store, kmax):
    bins, nd = 9, 10
    t = _targets(bins)
    below_one = float(np.nextafter(1.0, 0.0))
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        ctx.rescore(t, SIZES, [0] * 3)
        median_ks = float(ctx.select(abi.ACCEPT_RESCORED, fractions=(0.5,)).values[0, 0])
        thr = [[1.0, INF, INF, INF], [below_one, INF, INF, INF], [INF] * 4, [median_ks, INF, INF, INF]]
        summ = ctx.download().summaries
        headers, _ = ctx.download_kept()
        nk = _nk(headers)
        got = ctx.accept_draws(t, SIZES, thr, nd, 3)
        part = ctx.accept_draws(t, SIZES, thr, nd, 3, [0, 2])
    bad, free = summ["error"] != 0, summ["error"] == 0
    # where every participating target takes the whole kept sample, every draw says the same
    whole_all, whole_90 = nk <= 90, nk <= 130
    assert (whole_all & free).sum() >= 10 and (~whole_90 & free).sum() >= 100
    assert np.all(np.isin(got.passes[whole_all], (0, nd))) and np.all(np.isin(part.passes[whole_all], (0, nd)))
    assert ((got.passes[~whole_90][:, 3] % nd) != 0).any()  # ... and elsewhere they differ
    assert not got.passes[bad].any() and np.all(got.passes[free][:, 2] == nd)
    empty = (nk == 0) & free
    assert empty.sum() >= 3  # {0, 0}: ks = 1.0 exactly — a tie at 1.0 passes, anything below fails
    assert np.all(got.passes[empty][:, 0] == nd) and not got.passes[empty][:, 1].any()


@pytest.mark.gpu
def test_guard_headers_pass_as_their_all_zero_records(engine_mod):
    """The state of tests/test_gpu_sample_states.py::test_end_to_end_at_the_size_guard: every kept header is the
    guard's, every record all zero — four zero distances pass every row, as in the loop."""
    from support.state_specs import E2E_BINS, _e2e_spec

    spec = _e2e_spec("bins", {0: 2**32 - 3, 1: 2}, max_cells=10, cell_cap=64)
    t = _targets(E2E_BINS, 2)
    thr = [[0.0, 0.0, 0.0, 0.0], [INF] * 4]
    with _launched(engine_mod, spec) as ctx:
        free = ctx.download().summaries["error"] == 0
        headers, _ = ctx.download_kept()
        assert np.all(headers["nminus"] == abi.KEPT_GUARD) and np.all(headers["nplus"] == abi.KEPT_GUARD)
        bits, counts = _loop(ctx, "keep", t, (200, 1), thr, (62, 63), (None,))[None]
        got = ctx.accept_draws(t, (200, 1), thr, 2, 62)
        np.testing.assert_array_equal(got.passes, bits.sum(axis=0))
        np.testing.assert_array_equal(got.sums, counts.sum(axis=0))
        assert free.any() and np.all(got.passes[free] == 2) and not got.passes[~free].any()


# ---- 9. refusals ----


@pytest.mark.gpu
def test_refusals(engine_mod):
    L = engine_mod.lib()
    bins, m = 9, 20
    hists = np.ones((65, bins), dtype=np.uint64)
    two = np.ascontiguousarray(hists[:2])
    ok_thr = [[0.5, INF, 0.0, 1.0]]
    base = dict(n_replicates=4, max_cells=50, hist_bins=bins, flags=abi.FLAG_REP_STATS)

    def call(ctx, *a, **kw):
        blk, keep = _block(*a, **kw)
        rc = L.ecdna_ssa_ctx_accept_draws(ctx.h, C.byref(blk))
        return rc, L.ecdna_ssa_last_error_message().decode()

    def refused(ctx, word, *a, **kw):
        rc, msg = call(ctx, *a, **kw)
        assert rc == abi.E_INVALID and word in msg, (word, rc, msg)

    with engine_mod.Context(abi.RunSpec(keep_cells=m, **base)) as ctx:
        refused(ctx, "sample_cells[1]", two, (5, m + 1), ok_thr)  # a bad block is refused before the state is looked at
        assert call(ctx, two, (5, m), ok_thr)[0] == abi.E_STATE  # before a launch
        assert L.ecdna_ssa_ctx_download_accept_draws(ctx.h, None, None) == abi.E_STATE
        ctx.launch()
        ctx.sync()
        assert L.ecdna_ssa_ctx_download_accept_draws(ctx.h, None, None) == abi.E_STATE  # before a call
        assert L.ecdna_ssa_ctx_accept_draws(ctx.h, None) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_accept_draws(None, None) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_download_accept_draws(None, None, None) == abi.E_INVALID
        refused(ctx, "struct_size", two, (5, 5), ok_thr, struct_size=C.sizeof(abi.AcceptDraws) + 8)
        refused(ctx, "reserved", two, (5, 5), ok_thr, reserved=1)
        refused(ctx, "timepoints", two, (5, 5), ok_thr, timepoints=2)
        refused(ctx, "n_targets", two, (5, 5), ok_thr, n_targets=0)
        refused(ctx, "n_targets", hists, (5,) * 65, ok_thr)
        blk, keep = _block(two, (5, 5), ok_thr)
        blk.target_hists = None
        assert L.ecdna_ssa_ctx_accept_draws(ctx.h, C.byref(blk)) == abi.E_INVALID
        assert b"target_hists is NULL" in L.ecdna_ssa_last_error_message()
        holed = two.copy()
        holed[1] = 0
        refused(ctx, "target_hists[1]", holed, (5, 5), ok_thr)
        refused(ctx, "sample_cells is NULL", two, None, ok_thr)
        refused(ctx, "sample_cells[0]", two, (0, 5), ok_thr)
        rc, msg = call(ctx, two, (5, m + 1), ok_thr)
        assert rc == abi.E_INVALID and "sample_cells[1]" in msg and "keep_cells = 20" in msg
        refused(ctx, "n_draws", two, (5, 5), ok_thr, n_draws=0)
        refused(ctx, "n_draws", two, (5, 5), ok_thr, n_draws=65)
        refused(ctx, "first_draw", two, (5, 5), ok_thr, first_draw=1)  # 1 + 64 > 64
        refused(ctx, "first_draw", two, (5, 5), ok_thr, first_draw=64, n_draws=1)
        refused(ctx, "first_draw", two, (5, 5), ok_thr, first_draw=0xFFFFFFFF, n_draws=2)
        refused(ctx, "n_thresholds", two, (5, 5), ok_thr, n_thresholds=0)
        refused(ctx, "n_thresholds", two, (5, 5), np.ones((33, 4)))
        blk, keep = _block(two, (5, 5), ok_thr)
        blk.thresholds = None
        assert L.ecdna_ssa_ctx_accept_draws(ctx.h, C.byref(blk)) == abi.E_INVALID
        assert b"thresholds is NULL" in L.ecdna_ssa_last_error_message()
        refused(ctx, "thresholds[1].entropy_rel", two, (5, 5), [[0, 0, 0, 0], [0.5, INF, -1e-300, 1.0]])
        refused(ctx, "thresholds[0].ks", two, (5, 5), [[np.nan, 0, 0, 0]])
        refused(ctx, "timepoint_mask", two, (5, 5), ok_thr, timepoint_mask=0b100)
        rc, msg = call(ctx, two, (5, 5), ok_thr, timepoints=1)  # a keep context has no timepoint block
        assert rc == abi.E_STATE and "create_keep_timepoints" in msg
        with pytest.raises(engine_mod.EngineError, match="sample_cells"):
            ctx.accept_draws(two, (5, m + 1), ok_thr)
        with pytest.raises(ValueError):
            ctx.accept_draws(two, (5, 5), ok_thr, store="snapshots")
        assert call(ctx, two, (5, m), ok_thr, first_draw=63, n_draws=1, timepoint_mask=0b10)[0] == abi.OK
        got = ctx.accept_draws(two, (5, m), [[INF] * 4] * 32, 64)  # ... and a good block is taken
        assert got.passes.shape == (4, 32) and np.all(got.passes == 64) and np.all(got.sums == 4 * 64)
    with engine_mod.Context(abi.RunSpec(**base)) as ctx:  # a context without either block
        ctx.launch()
        ctx.sync()
        rc, msg = call(ctx, two, (5, 5), ok_thr)
        assert rc == abi.E_STATE and "ecdna_ssa_ctx_create_keep" in msg
        assert call(ctx, two, (5, 5), ok_thr, timepoints=1)[0] == abi.E_STATE
    spec = abi.RunSpec(snapshots=(10, 30), snapshot_stats=True, keep_timepoint_cells=m, **base)
    with engine_mod.Context(spec) as ctx:
        three = np.ascontiguousarray(hists[:3])
        refused(ctx, "n_targets must be T = 2", three, (5, 5, 5), ok_thr, timepoints=1)
        refused(ctx, "n_targets must be T = 2", hists[:1], (5,), ok_thr, timepoints=1)
        assert call(ctx, two, (5, m), ok_thr, timepoints=1)[0] == abi.E_STATE  # before a launch
        rc, msg = call(ctx, two, (5, m), ok_thr)  # ... and it has no keep block
        assert rc == abi.E_STATE and "ecdna_ssa_ctx_create_keep" in msg
        ctx.launch()
        ctx.sync()
        refused(ctx, "timepoint_mask", two, (5, m), ok_thr, timepoints=1, timepoint_mask=0b100)
        refused(ctx, "sample_cells[1]", two, (5, m + 1), ok_thr, timepoints=1)
        assert call(ctx, two, (5, m), ok_thr, timepoints=1, timepoint_mask=0b10)[0] == abi.OK
        assert ctx.accept_draws(two, (5, m), ok_thr, 3, 61, store="timepoints").passes.shape == (4, 1)
