"""The accepted thinnings pooled (ecdna_ssa_ctx_pool_draws; thinned pooling mapping v1, include/ecdna_ssa.h, DESIGN.md
§3.4) on the GPU.

The mapping's contracts are equalities of integers. K1 is checked against the loop the call replaces — per draw the
sized rescore, the acceptance pass and pool_accepted — and everything, out_thinned included, against the numpy
restatement (tests/pool_draws_law.py) at thresholds that lie in gaps of the law's own distances, so that the float
tolerance of the records cannot flip a verdict. The fixtures are those of tests/test_gpu_accept_draws.py."""
import ctypes as C

import numpy as np
import pytest

import accept_draws_law as adl
import accept_law as al
import keep_law as kl
import pool_draws_law as pdl
import thin_law as tl
from ecdna_evo_amd import abi
from support.draws_specs import (FRACTIONS, INF, KEEP, N, PER_SET, SEED, SETS, SIZES, TWO_STORES, _block,
                                 _gap_thresholds, _nk, _rows, _spec, _targets)
from support.gpu import _flags, _launched


def _sets(ids, per_set=PER_SET):
    return (np.asarray(ids, dtype=np.uint64) // np.uint64(per_set)).astype(np.int64)


def _partial_rows(passes, nd, rows):
    """Of `rows`, those under which some replicate passes some but not all of the nd draws, most such replicates
    first."""
    c = ((passes > 0) & (passes < nd)).sum(axis=0)
    return [int(q) for q in sorted(rows, key=lambda q: -c[q]) if c[q] > 0]


def _three_rows(ctx, t, sizes, thr, tps):
    """thr with its rows rearranged so that three kinds of row can be named: (rows, a partial row, the all-+inf row 30,
    the partial last row 31); partial under every set of timepoints of tps."""
    both = [ctx.accept_draws(t, sizes, thr, 64, 0, list(tp) if tp else None).passes for tp in tps]
    part = [q for q in _partial_rows(both[0], 64, range(30)) if all(_partial_rows(p, 64, [q]) for p in both)]
    assert len(part) >= 2, "the fixture has no two rows that decide differently from draw to draw"
    thr = thr.copy()
    thr[31] = thr[part[1]]
    thr[30] = INF
    return thr, part[0], 30, 31


def _loop_pools(ctx, store, t, sizes, thr, draws, tp, rows):
    """The loop the call replaces: per draw the sized rescore, the accept and, per row, pool_accepted.
    [D][rows][slices][sets][bins] u64."""
    out = []
    for d in draws:
        if store == "keep":
            ctx.rescore(t, sizes, [d] * len(sizes))
            ctx.accept(abi.ACCEPT_RESCORED, thr, list(tp) if tp else None)
            out.append([ctx.pool_accepted(q)[None] for q in rows])
        else:
            ctx.rescore_timepoints(t, sizes, d)
            ctx.accept(abi.ACCEPT_RESCORED_TIMEPOINTS, thr, list(tp) if tp else None)
            out.append([ctx.pool_accepted_timepoints(q) for q in rows])
    return np.asarray(out, dtype=np.uint64)


# ---- 1. K1 against the existing loop ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("bins", [9, 130])
def test_kept_equals_the_loop_of_rescore_accept_and_pool(engine_mod, store, kmax, bins):
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        ctx.rescore(t, SIZES, [0] * 3)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        tps = (None, (0, 2))
        thr, partial, inf_row, last = _three_rows(ctx, t, SIZES, thr, tps)
        rows = (partial, inf_row, last)
        assert np.all(np.isinf(thr[inf_row])) and last == len(thr) - 1 == 31
        for tp in tps:
            tpl = list(tp) if tp else None
            passes = ctx.accept_draws(t, SIZES, thr, 64, 0, tpl).passes
            for q in (partial, last):  # the row is non-trivial
                assert ((passes[:, q] > 0) & (passes[:, q] < 64)).any(), (tp, q)
            assert passes[:, inf_row].max() == 64
            loop = _loop_pools(ctx, "keep", t, SIZES, thr, range(64), tp, rows)
            for first, nd in ((0, 64), (61, 3)):
                for j, q in enumerate(rows):
                    got = ctx.pool_draws(t, SIZES, thr, q, nd, first, tpl)
                    assert got.kept.shape == (1, SETS, bins) and got.thinned.shape == (3, SETS, bins)
                    assert got.kept.dtype == got.thinned.dtype == np.uint64
                    np.testing.assert_array_equal(got.kept, loop[first:first + nd, j].sum(axis=0, dtype=np.uint64),
                                                  err_msg=f"timepoints {tp}, draws {first}..{first + nd - 1}, row {q}")
                    assert got.kept.sum() > 0


# ---- 2. equals the restatement ----

def _gap_rows(per_draw, free):
    picks = (0.1, 0.35, 0.6, 0.9)
    cuts = [_gap_thresholds(np.concatenate([r[f][free].ravel() for r in per_draw]), picks) for f in al.FIELDS]
    return [[cuts[x][(q + x) % 4] if (q >> x) & 1 else INF for x in range(4)] for q in range(16)]


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
        hists = pdl.thinned_hists(slots, ids, bins, first, nd)
        thr = _gap_rows(per_draw, summ["error"] == 0)
        partial = 0
        for tp in (None, [1], [0, 2]):
            mask = sum(1 << p for p in tp) if tp else 0
            for q in (3, 6, 15):
                want_t, want_k, passes = pdl.pool_draws(slots, [(headers, cells)], summ, ids, bins, PER_SET, SETS, thr,
                                                        q, first, nd, mask, per_draw, hists)
                got = ctx.pool_draws(t, SIZES, thr, q, nd, first, tp)
                np.testing.assert_array_equal(got.thinned, want_t, err_msg=f"timepoints {tp}, row {q}: thinned")
                np.testing.assert_array_equal(got.kept, want_k, err_msg=f"timepoints {tp}, row {q}: kept")
                partial += int(((passes > 0) & (passes < nd)).sum())
                if tp == [0, 2]:  # slot 1 is held out of the verdict and still predicted
                    assert passes.any() and got.thinned[1].sum() > 0
                    assert (got.thinned[1] != got.thinned[0]).any()
        assert partial > 0


# ---- 3. K2, K3 and K4 on the device ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_whole_slot_equals_kept_and_bin_sums(engine_mod, store, kmax):
    bins, sizes = 33, (KEEP, 90, 90)
    t = _targets(bins)
    spec = _spec(store, kmax, bins)
    sets = _sets(spec.replicate_ids())
    with _launched(engine_mod, spec) as ctx:
        headers, _ = ctx.download_kept()
        ctx.rescore(t, sizes, [0] * 3)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        passes = ctx.accept_draws(t, sizes, thr, 64, 0).passes
        rows = _partial_rows(passes, 64, range(32))[:2] + [31]
        assert len(rows) == 3
        for q in rows:
            got = ctx.pool_draws(t, sizes, thr, q, 64, 0)
            np.testing.assert_array_equal(got.thinned[0], got.kept[0], err_msg=f"K2, row {q}")
            np.testing.assert_array_equal(got.thinned[1], got.thinned[2], err_msg=f"K4, row {q}")
            assert (got.thinned[1] != got.thinned[0]).any()
            guard = (headers["nminus"] == abi.KEPT_GUARD) & (headers["nplus"] == abi.KEPT_GUARD)
            nk = np.where(guard, 0, _nk(headers))
            for slot, m1 in enumerate(sizes):
                want = np.bincount(sets, weights=passes[:, q].astype(np.int64) * np.minimum(m1, nk), minlength=SETS)
                np.testing.assert_array_equal(got.thinned[slot].sum(axis=1), want.astype(np.uint64),
                                              err_msg=f"K3, row {q}, slot {slot}")


# ---- 4. the snapshot timepoint store ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_snapshot_timepoints(engine_mod, store, kmax):
    """Untaken snapshots, two timepoints scored whole (10 and 30 cells below their m1 = 20 and 50) and one thinned (35
    of 50 kept cells)."""
    bins, m, sizes = 33, 50, (20, 50, 35)
    t = _targets(bins)
    spec = _spec(store, kmax, bins, keep_cells=None, snapshots=(10, 30, 100), snapshot_stats=True,
                 keep_timepoint_cells=m)
    ids = spec.replicate_ids()
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        headers, cells = ctx.download_kept_timepoints()
        taken = _nk(headers) > 0
        assert taken[0].sum() >= 150 and not taken[2].all() and taken[2].sum() >= 30
        # K1 against the loop of rescore_timepoints, accept and pool_accepted_timepoints
        ctx.rescore_timepoints(t, sizes, 0)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=FRACTIONS).values)
        first, nd = 40, 12
        for tp in (None, (0, 2), (1,)):
            tpl = list(tp) if tp else None
            passes = ctx.accept_draws(t, sizes, thr, nd, first, tpl, store="timepoints").passes
            part = _partial_rows(passes, nd, range(32))
            rows = (part[0] if part else 29, 31)
            assert part or tp == (1,)  # (timepoint 1 alone is scored whole: every draw says the same)
            loop = _loop_pools(ctx, "timepoints", t, sizes, thr, range(first, first + nd), tp, rows)
            for j, q in enumerate(rows):
                got = ctx.pool_draws(t, sizes, thr, q, nd, first, tpl, store="timepoints")
                assert got.kept.shape == got.thinned.shape == (3, SETS, bins)
                np.testing.assert_array_equal(got.kept, loop[:, j].sum(axis=0, dtype=np.uint64),
                                              err_msg=f"timepoints {tp}, row {q}")
                # the whole-scored timepoints pool their kept samples (K2 per replicate: a + b <= m1 there)
                np.testing.assert_array_equal(got.thinned[0], got.kept[0])
                np.testing.assert_array_equal(got.thinned[1], got.kept[1])
                assert got.kept.sum() > 0
        # ... and against the restatement, every slice on its own snapshot's stream
        first, nd = 5, 3
        slots = [adl.Slot(headers[s], cells[s], t[s], sizes[s], SEED, snapshot=s) for s in range(3)]
        slices = [(headers[s], cells[s]) for s in range(3)]
        per_draw = [adl.records(slots, ids, bins, d) for d in range(first, first + nd)]
        hists = pdl.thinned_hists(slots, ids, bins, first, nd)
        thr = _gap_rows(per_draw, summ["error"] == 0)
        partial = 0
        for tp in (None, [2], [0, 1]):
            mask = sum(1 << p for p in tp) if tp else 0
            for q in (0, 6, 15):  # (row 0 switches everything off)
                want_t, want_k, passes = pdl.pool_draws(slots, slices, summ, ids, bins, PER_SET, SETS, thr, q, first,
                                                        nd, mask, per_draw, hists)
                got = ctx.pool_draws(t, sizes, thr, q, nd, first, tp, store="timepoints")
                np.testing.assert_array_equal(got.thinned, want_t, err_msg=f"timepoints {tp}, row {q}: thinned")
                np.testing.assert_array_equal(got.kept, want_k, err_msg=f"timepoints {tp}, row {q}: kept")
                partial += int(((passes > 0) & (passes < nd)).sum())
                if tp == [0, 1] and q == 0:  # timepoint 2 is held out of the verdict and still predicted, thinned
                    assert got.thinned[2].sum() > 0 and (got.thinned[2] != got.kept[2]).any()
        assert partial > 0


# ---- 5. the passage store ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_passage_timepoints(engine_mod, store, kmax):
    """Two growth phases passaged at 100 cells, 40 measured of each: every phase pools under its own key seed_g, and the
    error rule holds per participating phase — a replicate with an error in phase 1 only pools nothing under the mask
    None, and pools both its phases' samples under the mask (0,)."""
    bins, m, sizes, G, nd = 33, 100, (40, 40), 2, 3
    t = _targets(bins, G)
    spec = _spec(store, kmax, bins, keep_cells=None, max_cells=500, max_time=None, init={0: 2, 1: 2, 12: 1},
                 cell_cap=1024, n_passages=G, passage_cells=m, passage_targets=t, keep_timepoint_cells=m)
    ids = spec.replicate_ids()
    sets = _sets(ids)
    with _launched(engine_mod, spec) as ctx:
        err = ctx.download().passages.summaries["error"]  # [G][n]
        only1 = (err[0] == 0) & (err[1] != 0)
        assert only1.any() and (err.sum(axis=0) == 0).sum() >= 100
        headers, cells = ctx.download_kept_timepoints()
        slots = [adl.Slot(headers[g], cells[g], t[g], sizes[g], tl.phase_key(SEED, g)) for g in range(G)]
        hists = pdl.thinned_hists(slots, ids, bins, 0, nd)  # [G][n][nd][bins]
        assert (hists[0].sum(axis=2) == np.minimum(sizes[0], _nk(headers[0]))[:, None])[err[0] == 0].all()
        inf = [[INF] * 4]
        for tp, ok in ((None, err.sum(axis=0) == 0), ((0,), err[0] == 0), ((1,), err[1] == 0)):
            got = ctx.pool_draws(t, sizes, inf, 0, nd, 0, list(tp) if tp else None, store="timepoints")
            for g in range(G):
                want_t = np.zeros((SETS, bins), dtype=np.uint64)
                want_k = np.zeros((SETS, bins), dtype=np.uint64)
                for i in np.flatnonzero(ok):
                    want_t[sets[i]] += hists[g, i].sum(axis=0, dtype=np.uint64)
                    h = (int(headers[g][i]["nminus"]), int(headers[g][i]["nplus"]))
                    want_k[sets[i]] += np.uint64(nd) * kl.kept_hist(h, cells[g][i], bins)
                np.testing.assert_array_equal(got.thinned[g], want_t, err_msg=f"timepoints {tp}, phase {g}: thinned")
                np.testing.assert_array_equal(got.kept[g], want_k, err_msg=f"timepoints {tp}, phase {g}: kept")
            # (the weights behind it: an error in phase 1 only counts where phase 1 takes part)
            w = ctx.accept_draws(t, sizes, inf, nd, 0, list(tp) if tp else None, store="timepoints").passes[:, 0]
            assert np.all(w[only1] == (nd if tp == (0,) else 0)) and np.all(w[ok] == nd) and not w[~ok].any()
        # K1 on a row that decides
        ctx.rescore_timepoints(t, sizes, 0)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=FRACTIONS).values, Q=12)
        passes = ctx.accept_draws(t, sizes, thr, 8, 0, None, store="timepoints").passes
        rows = _partial_rows(passes, 8, range(12))[:1]
        assert rows
        loop = _loop_pools(ctx, "timepoints", t, sizes, thr, range(8), None, rows)
        got = ctx.pool_draws(t, sizes, thr, rows[0], 8, 0, None, store="timepoints")
        np.testing.assert_array_equal(got.kept, loop[:, 0].sum(axis=0, dtype=np.uint64))


# ---- 6. the limits of the plan ----

def _limit_case(store, kmax, case):
    """(spec, bins, m1, seed, per_set, n_sets) of eight replicates at a limit of the LDS plan."""

    if case == "largest":  # pure birth to 8,200 cells: every kept sample is full
        spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=8, max_cells=8200, hist_bins=2048,
                           flags=_flags(store), bin_kmax=kmax, keep_cells=4096)
        return spec, 2048, 2048, 3, 8, 1
    return _spec(store, kmax, 2, n_replicates=8), 2, 90, SEED, PER_SET, SETS


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("case", ["largest", "smallest"])
def test_limits(engine_mod, store, kmax, case):
    """The largest table (m' = 2048 of 4,096 kept cells) beside the largest histogram (2,048 bins), one wave per
    workgroup; and the smallest histogram, two bins."""
    spec, bins, m1, seed, per_set, n_sets = _limit_case(store, kmax, case)
    rng = np.random.default_rng(9)
    t = rng.integers(1, 50, (1, bins)).astype(np.uint64)
    ids = spec.replicate_ids()
    first, nd = 62, 2
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        headers, cells = ctx.download_kept()
        nk = _nk(headers)
        assert case != "largest" or np.all(nk == 4096)
        slots = [adl.Slot(headers, cells, t[0], m1, seed)]
        per_draw = [adl.records(slots, ids, bins, d) for d in range(first, first + nd)]
        hists = pdl.thinned_hists(slots, ids, bins, first, nd)
        ks = np.concatenate([r["ks"][summ["error"] == 0].ravel() for r in per_draw])
        thr = [[_gap_thresholds(ks, (0.5,))[0], INF, INF, INF], [INF] * 4]
        for q in (0, 1):
            want_t, want_k, passes = pdl.pool_draws(slots, [(headers, cells)], summ, ids, bins, per_set, n_sets, thr, q,
                                                    first, nd, 0, per_draw, hists)
            got = ctx.pool_draws(t, (m1,), thr, q, nd, first)
            np.testing.assert_array_equal(got.thinned, want_t, err_msg=f"row {q}: thinned")
            np.testing.assert_array_equal(got.kept, want_k, err_msg=f"row {q}: kept")
            assert 0 < passes.sum() and (q == 1 or passes.sum() < 8 * nd)
            assert got.thinned.sum() == (passes * np.minimum(m1, nk)).sum() > 0  # K3


# ---- 7. independence ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_nothing_else_moves(engine_mod, store, kmax):
    bins = 33
    t = _targets(bins)
    L = engine_mod.lib()
    thr = [[0.5, INF, INF, INF], [INF, 0.3, INF, 0.2], [INF] * 4]

    def state(ctx):
        acc = ctx.download_accept()
        adr = ctx.download_accept_draws()
        sel = ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))
        return (ctx.download_rescored().tobytes(), acc.counts.tobytes(), acc.mask.tobytes(), acc.n_accepted,
                acc.ids.tobytes(), acc.stats.tobytes(), adr.sums.tobytes(), adr.passes.tobytes(), sel.population,
                sel.values.tobytes(), sel.counts_le.tobytes(), ctx.pool_accepted(1).tobytes())

    with engine_mod.Context(_spec(store, kmax, bins)) as ctx:
        blk, alive = _block(t, SIZES, thr, n_draws=8)
        out = np.zeros((3, SETS, bins), dtype=np.uint64)
        # before a launch
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, out.ctypes.data, None) == abi.E_STATE
        assert b"pool_draws before launch" in L.ecdna_ssa_last_error_message()
        ctx.launch()
        ctx.sync()
        # the call works with no earlier accept_draws or rescore, and leaves the store without records
        first = ctx.pool_draws(t, SIZES, thr, 0, 8)
        assert first.thinned.sum() > 0 and first.kept.sum() > 0
        assert L.ecdna_ssa_ctx_download_rescored(ctx.h, None) == abi.E_STATE
        assert L.ecdna_ssa_ctx_download_accept_draws(ctx.h, None, None) == abi.E_STATE
        # one output alone is the same array
        only_t, only_k = np.zeros_like(first.thinned), np.zeros_like(first.kept)
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, only_t.ctypes.data, None) == abi.OK
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, None, only_k.ctypes.data) == abi.OK
        assert only_t.tobytes() == first.thinned.tobytes() and only_k.tobytes() == first.kept.tobytes()
        ctx.rescore(t, (199, 60, 130), (1, 2, 3))
        ctx.select(abi.ACCEPT_RESCORED, fractions=(0.1, 0.5))  # (leaves cached keys)
        ctx.accept(abi.ACCEPT_RESCORED, thr, None, 1, 50)
        ctx.accept_draws(t, SIZES, thr, 8)
        before = state(ctx)
        again = ctx.pool_draws(t, SIZES, thr, 0, 8)
        assert again.thinned.tobytes() == first.thinned.tobytes() and again.kept.tobytes() == first.kept.tobytes()
        ctx.pool_draws(t[:1], (77,), _rows(np.full((4, 2), 0.25)), 31, 64, 0)  # (other sizes of every buffer)
        assert state(ctx) == before
        # a relaunch invalidates nothing of this call: it holds no result
        ctx.launch()
        ctx.sync()
        back = ctx.pool_draws(t, SIZES, thr, 0, 8)
        assert back.thinned.tobytes() == first.thinned.tobytes() and back.kept.tobytes() == first.kept.tobytes()
        # refusals on a launched context name the field
        for q, want in ((3, b"pool_draws.threshold"), (0xFFFFFFFF, b"pool_draws.threshold")):
            assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), q, out.ctypes.data, None) == abi.E_INVALID
            assert want in L.ecdna_ssa_last_error_message()
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, None, None) == abi.E_INVALID
        assert b"out_thinned" in L.ecdna_ssa_last_error_message()
        bad, alive2 = _block(t, (5, KEEP + 1, 5), thr)
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(bad), 0, out.ctypes.data, None) == abi.E_INVALID
        assert b"accept_draws.sample_cells[1]" in L.ecdna_ssa_last_error_message()
        blk.timepoints = 1  # a keep context has no timepoint block
        assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, out.ctypes.data, None) == abi.E_STATE
        assert b"create_keep_timepoints" in L.ecdna_ssa_last_error_message()
    base = dict(n_replicates=4, max_cells=50, hist_bins=bins, flags=abi.FLAG_REP_STATS)
    with engine_mod.Context(abi.RunSpec(**base)) as ctx:  # a context without either block
        ctx.launch()
        ctx.sync()
        for tpb in (0, 1):
            blk, alive = _block(t, (5, 5, 5), thr, timepoints=tpb)
            assert L.ecdna_ssa_ctx_pool_draws(ctx.h, C.byref(blk), 0, out.ctypes.data, None) == abi.E_STATE
            assert b"ecdna_ssa_ctx_create_keep" in L.ecdna_ssa_last_error_message()


# ---- 8. chunks and shards ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_placement_independence(engine_mod, store, kmax, monkeypatch, tmp_path):
    """The same run forced into several chunks gives identical arrays; two interleaved shards sum to the whole run's."""
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    bins = 33
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        ctx.rescore(t, SIZES, [0] * 3)
        thr = _rows(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values)
        q = _partial_rows(ctx.accept_draws(t, SIZES, thr, 24, 5).passes, 24, range(32))[0]
        whole = ctx.pool_draws(t, SIZES, thr, q, 24, 5)
        # shard.pool_draws over a process group of one
        assert not dist.is_initialized()
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            got = shard.pool_draws(ctx, t, SIZES, thr, q, 24, 5)
        finally:
            dist.destroy_process_group()
        np.testing.assert_array_equal(got.thinned, whole.thinned)
        np.testing.assert_array_equal(got.kept, whole.kept)
    assert whole.thinned.sum() > 0 and whole.kept.sum() > 0
    total_t, total_k = np.zeros_like(whole.thinned), np.zeros_like(whole.kept)
    for g in range(2):
        n = len(range(g, N, 2))
        with _launched(engine_mod, _spec(store, kmax, bins, first_replicate=g, replicate_stride=2,
                                         n_replicates=n)) as part:
            got = part.pool_draws(t, SIZES, thr, q, 24, 5)
        assert got.kept.sum() > 0
        total_t += got.thinned
        total_k += got.kept
    np.testing.assert_array_equal(total_t, whole.thinned)
    np.testing.assert_array_equal(total_k, whole.kept)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_spec(store, kmax, bins)) as ctx:
        assert ctx.instance()["n_chunks"] == 3
        ctx.launch()
        ctx.sync()
        got = ctx.pool_draws(t, SIZES, thr, q, 24, 5)
    assert got.thinned.tobytes() == whole.thinned.tobytes() and got.kept.tobytes() == whole.kept.tobytes()
