"""The kept samples rescored at each target's own number of measured cells (ecdna_ssa_rescore_t,
ecdna_ssa_ctx_rescore_sized and _rescore_timepoints_sized; thinning mapping v1, include/ecdna_ssa.h).

The kept samples themselves are pinned to their restatements by tests/test_gpu_keep.py and
tests/test_gpu_timepoint_keep.py; here they are downloaded and the sized records are compared with the numpy
restatement of the thinning (tests/thin_law.py) applied to them: `cells` exactly, floats at the ABC-statistics tolerance
(1e-12 relative, tests/test_gpu_abc_stats.py: sums are reduced in a different order on the GPU; log is ocml's vs
numpy's). Where the mapping promises bytes — the whole kept sample, no sizes, equal (m1, d), placement — bytes are
compared. One test checks the law itself, independently of the restatement, against the exact hypergeometric pmf."""
import ctypes as C

import numpy as np
import pytest

import accept_law as al
import keep_law as kl
import select_law as slw
import thin_law as tl
from ecdna_evo_amd import abi
from exact_law import chi2_lumped
from support.gpu import _flags, _launched, _same_accept, _same_select

RTOL, ATOL = 1e-12, 1e-14
FLOATS = ("mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")
INF = np.inf
TWO_STORES = [("rows", 0), ("bins", 64)]
SEED = 31
KEEP = 199  # odd: a row of 199 u16 is not 16-byte aligned; above 128: the picks need more than one 64-draw batch
# whole; picks over two batches; a complement with m' = 69; m1 = 1; a complement with m' = 1; a second stream
SIZES = (199, 90, 130, 1, 198, 60)
DRAWS = (0, 0, 0, 3, 0, 63)
P = len(SIZES)
_RUNS = {}


def _targets(bins, n=P):
    rng = np.random.default_rng(23)
    t = rng.integers(0, 70, (n, bins)).astype(np.uint64)
    t[:, 0] += 40
    t[:, bins - 1] = np.arange(n) % 4
    return t


def _spec(store, kmax, bins, **kw):
    """256 birth-death replicates from three cells to 600 cells or time 6: some go extinct, some end small, most end
    above the kept sample's size; the 12-copy cell lies above the last of 9 bins."""
    base = dict(seed=SEED, process=abi.BIRTH_DEATH, rates=((1.0, 1.3, 0.4, 0.4),), n_replicates=256, max_cells=600,
                max_time=6.0, hist_bins=bins, init={0: 1, 1: 1, 12: 1}, flags=_flags(store), bin_kmax=kmax,
                keep_cells=KEEP)
    base.update(kw)
    return abi.RunSpec(**base)


def _same_record(got, want, tag):
    assert int(got["cells"]) == want["cells"], f"{tag}: cells"
    for f in FLOATS:
        np.testing.assert_allclose(got[f], want[f], rtol=RTOL, atol=ATOL, err_msg=f"{tag}: {f}")


def _check_against_law(rec, headers, cells, sizes, draws, targets, key, ids, bins, snapshot=None, tag=""):
    """rec [P][n] against thin_law.record of every (target, replicate)."""
    for p in range(len(sizes)):
        for i in range(len(ids)):
            h = (int(headers[i]["nminus"]), int(headers[i]["nplus"]))
            want = tl.record(h, cells[i], sizes[p], key, int(ids[i]), bins, targets[p], draws[p], snapshot)
            _same_record(rec[p][i], want, f"{tag} target {p}, replicate {i}, header {h}")


def _whole_run(engine_mod, store, kmax, bins):
    """The whole run's kept samples, its unsized records and its sized records: one per key, shared, left unchanged."""
    key = (store, kmax, bins)
    if key not in _RUNS:
        t = _targets(bins)
        with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
            headers, cells = ctx.download_kept()
            plain = ctx.rescore(t)
            sized = ctx.rescore(t, SIZES, DRAWS)
        _RUNS[key] = (headers, cells, plain, sized)
    return _RUNS[key]


# ---- 1. records against the restatement ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
@pytest.mark.parametrize("bins", [9, 33])
def test_sized_records_match_the_restatement(engine_mod, store, kmax, bins):
    t = _targets(bins)
    headers, cells, plain, sized = _whole_run(engine_mod, store, kmax, bins)
    spec = _spec(store, kmax, bins)
    assert sized.dtype == abi.STATS_DTYPE and sized.shape == (P, 256)
    nk = headers["nminus"].astype(np.int64) + headers["nplus"]
    assert not (headers["nplus"] == abi.KEPT_GUARD).any()
    # the hard cases occur: {0, 0}, kept samples smaller than every thinned size but 1, and full ones
    empty, small = nk == 0, (nk > 0) & (nk < 60)
    assert empty.sum() >= 3 and small.sum() >= 10 and (nk == KEEP).sum() >= 100 and ((nk >= 60) & (nk < KEEP)).sum() >= 20
    assert bins == 33 or ((cells > bins - 1) & (np.arange(KEEP)[None, :] < headers["nplus"][:, None])).any()
    _check_against_law(sized, headers, cells, SIZES, DRAWS, t, SEED, spec.replicate_ids(), bins)
    # a thinned sample has its size; a target whose size reaches the kept sample's takes it whole: rescore's bytes
    for p, m1 in enumerate(SIZES):
        np.testing.assert_array_equal(sized[p]["cells"], np.minimum(nk, m1), err_msg=f"target {p}")
        whole = nk <= m1
        assert whole[empty].all() and (m1 == 1 or whole[small].all())
        assert sized[p][whole].tobytes() == plain[p][whole].tobytes(), p
    assert sized[0].tobytes() == plain[0].tobytes()  # m1 = keep_cells
    # ... and the thinned records are not the whole sample's
    for p in (1, 2, 3, 5):
        assert (sized[p][nk == KEEP]["mean"] != plain[p][nk == KEEP]["mean"]).mean() > 0.9, p


# ---- 2. bytes where bytes are promised ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_bytes_where_bytes_are_promised(engine_mod, store, kmax):
    bins = 33
    t = _targets(bins)
    with _launched(engine_mod, _spec(store, kmax, bins)) as ctx:
        plain = ctx.rescore(t)
        assert ctx.rescore(t, None, (0,) * P).tobytes() == plain.tobytes()  # no sizes: the unsized call's records
        assert ctx.rescore(t, None, DRAWS).tobytes() == plain.tobytes()  # (a draw with nothing thinned has no effect)
        assert ctx.rescore(t, KEEP).tobytes() == plain.tobytes()  # every target on keep_cells cells
        assert ctx.rescore(t, (KEEP,) * P, DRAWS).tobytes() == plain.tobytes()
        assert ctx.accept_timepoints(abi.ACCEPT_RESCORED) == P
        # targets 1 and 2 with equal (m1, d) and equal histograms: equal bytes; target 4 differs in d alone
        t2 = t.copy()
        t2[2] = t2[1]
        t2[4] = t2[1]
        rec = ctx.rescore(t2, (199, 90, 90, 1, 90, 60), (0, 7, 7, 3, 8, 63))
        assert rec[1].tobytes() == rec[2].tobytes()
        assert ctx.download_rescored().tobytes() == rec.tobytes()
        headers, _ = ctx.download_kept()
        full = headers["nminus"].astype(np.int64) + headers["nplus"] > 90
        differ = (rec[1]["mean"] != rec[4]["mean"]) | (rec[1]["ks"] != rec[4]["ks"])
        assert full.sum() >= 100 and differ[full].mean() > 0.9 and not differ[~full].any()
        # d = 0 and d = 1 at the same m1, each alone
        a, b = ctx.rescore(t[:1], 90, 0), ctx.rescore(t[:1], 90, 1)
        differ = (a[0]["mean"] != b[0]["mean"]) | (a[0]["ks"] != b[0]["ks"])
        assert differ[full].mean() > 0.9 and a[0][~full].tobytes() == b[0][~full].tobytes()
        assert ctx.rescore(t[:1], 90, 0).tobytes() == a.tobytes()  # the same call again: the same records


# ---- 3. placement ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_placement_independence(engine_mod, store, kmax, monkeypatch):
    """Three interleaved shards, and forced chunks, give the whole run's sized records byte for byte."""
    bins = 33
    t = _targets(bins)
    _, _, _, whole = _whole_run(engine_mod, store, kmax, bins)
    for g in range(3):
        n = len(range(g, 256, 3))
        with _launched(engine_mod, _spec(store, kmax, bins, first_replicate=g, replicate_stride=3,
                                         n_replicates=n)) as part:
            rec = part.rescore(t, SIZES, DRAWS)
        for p in range(P):
            assert rec[p].tobytes() == whole[p][g::3].tobytes(), (g, p)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(_spec(store, kmax, bins)) as ctx:
        assert ctx.instance()["n_chunks"] == 3
        ctx.launch()
        ctx.sync()
        assert ctx.rescore(t, SIZES, DRAWS).tobytes() == whole.tobytes()


# ---- 4. the law, independent of the restatement ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_thinned_sample_law_is_hypergeometric(engine_mod, store, kmax):
    """30 N- and 10 N+ cells, untouched (every replicate stops at MaxCells before its first event), 20 of them kept and
    8 of those measured: the N+ cells among the 8 are Hypergeometric(40, 10, 8), on draw 0 and on draw 5."""
    from scipy import stats

    n, m1 = 65536, 8
    spec = abi.RunSpec(seed=2024, process=abi.PURE_BIRTH, n_replicates=n, max_cells=40, hist_bins=17,
                       init={0: 30, 2: 10}, flags=abi.FLAG_REP_STATS | (abi.FLAG_BIN_STORE if store == "bins" else 0),
                       bin_kmax=kmax, keep_cells=20)
    target = np.ones((1, 17), dtype=np.uint64)
    seen = []
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        assert np.all(summ["iters"] == 0) and np.all(summ["nplus"] == 10)
        for d in (0, 5):
            rec = ctx.rescore(target, m1, d)[0]
            assert np.all(rec["cells"] == m1)
            x = np.rint(rec["frequency"] * m1).astype(np.int64)
            np.testing.assert_allclose(rec["frequency"] * m1, x, rtol=0, atol=1e-9)
            np.testing.assert_allclose(rec["mean"] * m1, 2 * x, rtol=0, atol=1e-9)  # every N+ cell has 2 copies
            obs = np.bincount(x, minlength=m1 + 1)
            assert len(obs) == m1 + 1
            p = chi2_lumped(obs, stats.hypergeom.pmf(np.arange(m1 + 1), 40, 10, m1) * n, min_expected=5)
            assert p > 1e-6, (d, p, obs.tolist())
            seen.append(x)
    assert (seen[0] != seen[1]).mean() > 0.3  # the two draws are two samples


# ---- 5. limits ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_limits(engine_mod, store, kmax):
    """The largest table (m' = 2048 of 4,096 kept cells) beside the largest histogram (2,048 bins): nothing is refused
    at launch and the records are the restatement's."""
    bins, m = 2048, 4096
    sizes, draws = (2048, 4095, 1), (0, 1, 63)
    rng = np.random.default_rng(9)
    t = rng.integers(0, 50, (3, bins)).astype(np.uint64)
    t[:, 0] += 1
    spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=bins,
                       flags=_flags(store), bin_kmax=kmax, keep_cells=m)
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        assert np.all(summ["nminus"] + summ["nplus"] == 8200) and not (summ["error"] != 0).any()
        headers, cells = ctx.download_kept()
        rec = ctx.rescore(t, sizes, draws)
    assert np.all(headers["nminus"].astype(np.int64) + headers["nplus"] == m)
    for p in range(3):
        assert np.all(rec[p]["cells"] == sizes[p])
    _check_against_law(rec, headers, cells, sizes, draws, t, 3, spec.replicate_ids(), bins)


# ---- 6. the size guard ----

@pytest.mark.gpu
@pytest.mark.parametrize("store", ["rows", "bins"])
def test_guard_headers_give_all_zero_records(engine_mod, store):
    """The state of tests/test_gpu_sample_states.py::test_end_to_end_at_the_size_guard (n- + n+ = 2^32 - 1): every kept
    header is the guard's, and every (m1, d) gives the all-zero record."""
    from support.state_specs import E2E_BINS, _e2e_spec

    spec = _e2e_spec(store, {0: 2**32 - 3, 1: 2}, max_cells=10, cell_cap=64)
    t = _targets(E2E_BINS, 4)
    with _launched(engine_mod, spec) as ctx:
        headers, _ = ctx.download_kept()
        assert np.all(headers["nminus"] == abi.KEPT_GUARD) and np.all(headers["nplus"] == abi.KEPT_GUARD)
        rec = ctx.rescore(t, (4096, 200, 1, 2048), (0, 0, 63, 5))
        assert rec.tobytes() == np.zeros((4, 64), dtype=abi.STATS_DTYPE).tobytes()
        assert ctx.rescore(t).tobytes() == rec.tobytes()


@pytest.mark.gpu
def test_a_sample_of_n_minus_cells_alone(engine_mod):
    """Two replicates of 50 N- cells, 20 kept: headers {20, 0}, no row to read, every thinned sample is N- cells."""
    bins = 9
    spec = abi.RunSpec(seed=5, process=abi.BIRTH_DEATH, n_replicates=2, max_cells=50, hist_bins=bins, init={0: 50},
                       flags=abi.FLAG_REP_STATS, keep_cells=20)
    t = _targets(bins, 3)
    sizes, draws = (5, 20, 19), (0, 0, 9)
    with _launched(engine_mod, spec) as ctx:
        headers, cells = ctx.download_kept()
        assert np.all(headers["nminus"] == 20) and np.all(headers["nplus"] == 0)
        rec = ctx.rescore(t, sizes, draws)
        plain = ctx.rescore(t)
    _check_against_law(rec, headers, cells, sizes, draws, t, 5, spec.replicate_ids(), bins)
    for p in range(3):
        assert np.all(rec[p]["cells"] == sizes[p]) and np.all(rec[p]["mean"] == 0.0) and np.all(rec[p]["frequency"] == 0.0)
        # (all cells alike: the thinned sample's distribution is the whole sample's)
        for f in ("entropy", "ks", "mean_rel", "entropy_rel", "frequency_diff"):
            np.testing.assert_array_equal(rec[p][f], plain[p][f], err_msg=f)


# ---- 7. timepoints ----

def _outputs(res):
    """Every array a download returned, by name, as bytes."""
    out = {}
    for owner, prefix in ((res, ""), (res.passages, "passages."), (res.cohort, "cohort.")):
        for name, v in (vars(owner) if owner is not None else {}).items():
            if isinstance(v, np.ndarray):
                out[prefix + name] = v.tobytes()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_snapshot_timepoints(engine_mod, store, kmax):
    """S = 2 snapshots at 60 and 300 cells, 50 cells kept of each: the first scored whole, the second on 20 cells, on the
    snapshot's own stream field with the thinning flag; nothing else moves."""
    bins, m, sizes = 33, 50, (50, 20)
    t = _targets(bins, 2)
    spec = abi.RunSpec(seed=SEED, process=abi.BIRTH_DEATH, rates=((1.0, 1.3, 0.4, 0.4),), n_replicates=256,
                       max_cells=400, hist_bins=bins, init={0: 1, 1: 1, 12: 1}, snapshots=(60, 300), snapshot_stats=True,
                       snapshot_targets=t, snapshot_subsample_cells=m,
                       flags=_flags(store) | abi.FLAG_SNAPSHOT_ROWS, bin_kmax=kmax, keep_timepoint_cells=m)
    ids = spec.replicate_ids()
    with _launched(engine_mod, spec) as ctx:
        before = _outputs(ctx.download(want_rows=True))
        headers, cells = ctx.download_kept_timepoints()
        plain = ctx.rescore_timepoints(t)
        for draw in (0, 7):
            rec = ctx.rescore_timepoints(t, sizes, draw)
            assert rec.dtype == abi.STATS_DTYPE and rec.shape == (2, 256)
            assert ctx.download_rescored_timepoints().tobytes() == rec.tobytes()
            assert ctx.accept_timepoints(abi.ACCEPT_RESCORED_TIMEPOINTS) == 2
            for s in range(2):
                _check_against_law(rec[s:s + 1], headers[s], cells[s], sizes[s:s + 1], (draw,), t[s:s + 1], SEED, ids,
                                   bins, snapshot=s, tag=f"snapshot {s}, draw {draw}")
            assert rec[0].tobytes() == plain[0].tobytes()  # m1 = keep_cells: the whole kept sample
            taken = headers[1]["nminus"].astype(np.int64) + headers[1]["nplus"] == m
            assert taken.sum() >= 100 and not taken.all()  # (extinct replicates never reach 300 cells: {0, 0})
            assert np.all(rec[1]["cells"][taken] == 20) and rec[1][~taken].tobytes() == plain[1][~taken].tobytes()
        assert ctx.rescore_timepoints(t, None, 9).tobytes() == plain.tobytes()  # no sizes: the unsized call's records
        # snapshot 1 on snapshot 0's field would be another sample: the field is the slice's own
        other = tl.record((int(headers[1][taken][0]["nminus"]), int(headers[1][taken][0]["nplus"])), cells[1][taken][0],
                          20, SEED, int(ids[taken][0]), bins, t[1], 7, snapshot=0)
        assert other["mean"] != rec[1][taken][0]["mean"] or other["ks"] != rec[1][taken][0]["ks"]
        h2, c2 = ctx.download_kept_timepoints()
        assert h2.tobytes() == headers.tobytes() and c2.tobytes() == cells.tobytes()
        assert _outputs(ctx.download(want_rows=True)) == before


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_passage_timepoints(engine_mod, store, kmax):
    """G = 3 growth phases passaged at 100 cells and measured at 30, 100 and 70: each phase under its own key; the
    founders and every launch-time output are unchanged by the call."""
    bins, m, sizes, G = 33, 100, (30, 100, 70), 3
    t = _targets(bins, G)
    spec = abi.RunSpec(seed=SEED, process=abi.BIRTH_DEATH, rates=((1.0, 1.3, 0.4, 0.4),), n_replicates=192,
                       max_cells=500, hist_bins=bins, init={0: 2, 1: 2, 12: 1}, cell_cap=1024, n_passages=G,
                       passage_cells=m, passage_targets=t, flags=_flags(store), bin_kmax=kmax, keep_timepoint_cells=m)
    ids = spec.replicate_ids()
    with _launched(engine_mod, spec) as ctx:
        before = _outputs(ctx.download())
        headers, cells = ctx.download_kept_timepoints()
        plain = ctx.rescore_timepoints(t)
        assert plain.tobytes() == ctx.download().passages.sample_stats.tobytes()
        for draw in (0, 63):
            rec = ctx.rescore_timepoints(t, sizes, draw)
            assert rec.shape == (G, 192) and ctx.download_rescored_timepoints().tobytes() == rec.tobytes()
            for g in range(G):
                _check_against_law(rec[g:g + 1], headers[g], cells[g], sizes[g:g + 1], (draw,), t[g:g + 1],
                                   tl.phase_key(SEED, g), ids, bins, tag=f"phase {g}, draw {draw}")
            assert rec[1].tobytes() == plain[1].tobytes()  # m1 = passage_cells: the founders themselves
            full = headers[0]["nminus"].astype(np.int64) + headers[0]["nplus"] == m
            assert full.sum() >= 100 and np.all(rec[0]["cells"][full] == 30)
        # phase 2 under phase 0's key would be another sample: the key is the slice's own
        j = int(np.flatnonzero(headers[2]["nminus"].astype(np.int64) + headers[2]["nplus"] == m)[0])
        other = tl.record((int(headers[2][j]["nminus"]), int(headers[2][j]["nplus"])), cells[2][j], 70, SEED,
                          int(ids[j]), bins, t[2], 63)
        assert other["mean"] != rec[2][j]["mean"] or other["ks"] != rec[2][j]["ks"]
        h2, c2 = ctx.download_kept_timepoints()
        assert h2.tobytes() == headers.tobytes() and c2.tobytes() == cells.tobytes()  # (phase 1's founders among them)
        assert _outputs(ctx.download()) == before


# ---- 8. downstream ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", TWO_STORES)
def test_through_accept_and_select(engine_mod, store, kmax):
    """Source 12 after a sized rescore: accept with thresholds that select chose equals the restatement of the
    acceptance on the downloaded records, and select's counts_le is the number a threshold at its value accepts."""
    bins = 33
    t = _targets(bins)
    spec = _spec(store, kmax, bins)
    with _launched(engine_mod, spec) as ctx:
        summ = ctx.download().summaries
        rec = ctx.rescore(t, SIZES, DRAWS)
        records = np.ascontiguousarray(rec.T)  # [n][P]
        for tp in ([1], [3], [1, 5], None):
            mask = sum(1 << p for p in tp) if tp else 0
            sel = ctx.select(abi.ACCEPT_RESCORED, fractions=(0.05, 0.3, 1.0), timepoints=tp)
            _same_select(sel, slw.select(records, summ, fractions=(0.05, 0.3, 1.0), timepoint_mask=mask), f"{tp}")
            assert sel.population == (summ["error"] == 0).sum()
            thr = [list(sel.values[:, j]) for j in range(3)]
            thr += [[sel.values[x, 1] if y == x else INF for y in range(4)] for x in range(4)]  # one distance each
            for q, cap in ((0, 0), (1, 40), (2, 256)):
                got = ctx.accept(abi.ACCEPT_RESCORED, thr, tp, q, cap)
                want = al.accept(records, summ, spec.n_replicates, spec.replicate_ids(), thr, 1, mask, q, cap)
                _same_accept(got, want, f"timepoints {tp}, row {q}")
                assert got.stats.tobytes() == records[want.index].tobytes()
            for x in range(4):  # select's contract: counts_le of them lie at or below the value
                assert got.counts[3 + x].sum() == sel.counts_le[x, 1], (tp, x)
            # (all four distances at once; the row of the largest values accepts every error-free replicate)
            assert got.counts[0].sum() <= got.counts[1].sum() <= got.counts[2].sum() == sel.population > 200


# ---- 9. refusals ----

def _block(hists, cells=None, draws=None, n=None):
    r = abi.Rescore(struct_size=C.sizeof(abi.Rescore), n_targets=hists.shape[0] if n is None else n)
    r.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    keep = [hists]
    if cells is not None:
        cells = np.ascontiguousarray(cells, dtype=np.uint32)
        r.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
        keep.append(cells)
    if draws is not None:
        draws = np.ascontiguousarray(draws, dtype=np.uint32)
        r.sample_draws = draws.ctypes.data_as(C.POINTER(C.c_uint32))
        keep.append(draws)
    return r, keep


@pytest.mark.gpu
def test_refusals(engine_mod):
    L = engine_mod.lib()
    bins, m = 9, 20
    hists = np.ones((65, bins), dtype=np.uint64)
    base = dict(n_replicates=4, max_cells=50, hist_bins=bins, flags=abi.FLAG_REP_STATS)

    def sized(ctx, *a, **kw):
        r, keep = _block(*a, **kw)
        rc = L.ecdna_ssa_ctx_rescore_sized(ctx.h, C.byref(r))
        return rc, L.ecdna_ssa_last_error_message().decode()

    with engine_mod.Context(abi.RunSpec(keep_cells=m, **base)) as ctx:
        two = hists[:2]
        assert sized(ctx, two, (5, 20))[0] == abi.E_STATE  # before a launch
        ctx.launch()
        ctx.sync()
        rc, msg = sized(ctx, two, (5, 0))
        assert rc == abi.E_INVALID and "sample_cells[1]" in msg  # m1 = 0
        rc, msg = sized(ctx, two, (m + 1, 5))
        assert rc == abi.E_INVALID and "sample_cells[0]" in msg and "keep_cells = 20" in msg
        rc, msg = sized(ctx, two, (5, 5), (0, 64))
        assert rc == abi.E_INVALID and "sample_draws[1]" in msg
        assert sized(ctx, two, None, (64, 0))[0] == abi.E_INVALID  # a draw above 63 is refused even where ignored
        rc, msg = sized(ctx, hists, (5,) * 65)
        assert rc == abi.E_INVALID and "n_targets" in msg  # P = 65
        assert sized(ctx, two, (5, 5), n=0)[0] == abi.E_INVALID
        holed = two.copy()
        holed[1] = 0
        rc, msg = sized(ctx, holed, (5, 5))
        assert rc == abi.E_INVALID and "target_hists[1]" in msg
        r, _ = _block(two, (5, 5))
        r.struct_size += 8
        assert L.ecdna_ssa_ctx_rescore_sized(ctx.h, C.byref(r)) == abi.E_INVALID
        r, _ = _block(two, (5, 5))
        r.reserved = 1
        assert L.ecdna_ssa_ctx_rescore_sized(ctx.h, C.byref(r)) == abi.E_INVALID
        r, _ = _block(two, (5, 5))
        r.target_hists = None
        assert L.ecdna_ssa_ctx_rescore_sized(ctx.h, C.byref(r)) == abi.E_INVALID
        assert L.ecdna_ssa_ctx_rescore_sized(ctx.h, None) == abi.E_INVALID
        with pytest.raises(engine_mod.EngineError, match="sample_cells"):
            ctx.rescore(two, (5, m + 1))
        with pytest.raises(engine_mod.EngineError, match="create_keep_timepoints"):
            ctx.rescore_timepoints(two, (5, 5))  # a keep context has no timepoint block
        assert sized(ctx, two, (5, m))[0] == abi.OK  # ... and a good block is taken
        rec = ctx.rescore(two, (5, m))
        assert rec.shape == (2, 4) and np.all(rec[0]["cells"] == 5) and np.all(rec[1]["cells"] == m)
    with engine_mod.Context(abi.RunSpec(**base)) as ctx:  # a context without the block
        ctx.launch()
        ctx.sync()
        rc, msg = sized(ctx, hists[:2], (5, 5))
        assert rc == abi.E_STATE and "ecdna_ssa_ctx_create_keep" in msg
        cells = np.asarray([5, 5], dtype=np.uint32)
        assert L.ecdna_ssa_ctx_rescore_timepoints_sized(ctx.h, hists.ctypes.data, cells.ctypes.data, 0) == abi.E_STATE
    spec = abi.RunSpec(snapshots=(10, 30), snapshot_stats=True, keep_timepoint_cells=m, **base)
    with engine_mod.Context(spec) as ctx:
        two = np.ascontiguousarray(hists[:2])
        cells = np.asarray([5, 20], dtype=np.uint32)

        def sized_tp(h, c, d):
            return L.ecdna_ssa_ctx_rescore_timepoints_sized(ctx.h, h.ctypes.data if h is not None else None,
                                                            c.ctypes.data if c is not None else None, d)

        assert sized_tp(two, cells, 0) == abi.E_STATE  # before a launch
        ctx.launch()
        ctx.sync()
        assert sized_tp(two, cells, 64) == abi.E_INVALID and sized_tp(two, None, 64) == abi.E_INVALID
        assert sized_tp(None, cells, 0) == abi.E_INVALID
        for bad in ((0, 5), (5, m + 1)):
            assert sized_tp(two, np.asarray(bad, dtype=np.uint32), 0) == abi.E_INVALID
            assert b"sample_cells" in L.ecdna_ssa_last_error_message()
        holed = two.copy()
        holed[0] = 0
        assert sized_tp(holed, cells, 0) == abi.E_INVALID and b"target_hists[0]" in L.ecdna_ssa_last_error_message()
        assert sized_tp(two, cells, 63) == abi.OK and sized_tp(two, None, 63) == abi.OK
        assert ctx.download_rescored_timepoints().shape == (2, 4)
