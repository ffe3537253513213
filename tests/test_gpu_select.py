"""ABC thresholds on the GPU (ecdna_ssa_ctx_select / ecdna_ssa_ctx_select_digits, select mapping v1; include/ecdna_ssa.h,
DESIGN.md §5 and §11).

Every comparison is exact: the population, the ranks, the values (as f64 bit patterns) and counts_le must equal the
numpy restatement (tests/select_law.py) applied to the same context's downloaded records, and ecdna_ssa_ctx_accept with
a selected value as its one threshold must accept exactly counts_le replicates — and fewer than the rank with the next
smaller double. The shapes are those of tests/test_gpu_accept.py (both take their spec builders from
tests/support/accept_specs.py): 3,000 or 192 replicates grown to 300 cells.

Each case first asserts its preconditions on the restatement: the population has at least two replicates and at least
two of the selected ks values differ, so no case is trivial; the passage case also selects a rank whose counts_le exceeds
it (a tie on the boundary). Two sizes cannot meet them as stated and assert what they can instead: with n_replicates = 1
the population is the one replicate, and the edge sizes, which run at K = 1, make two calls (ranks 1 and M) and compare
the two calls' ks values.

A NaN distance is not reachable from a run: the statistics never produce one (tests/test_gpu_accept.py found the same).
The NaN branch of the key map is therefore checked on the CPU only, through the header function the kernels call
(tests/test_select_native.py). A context's seed is fixed when it is created, so a relaunch reproduces its records: the
relaunch case checks that select still follows them and that a context with another seed follows its own.

One ECDNA_E_INVALID condition of the header, n_replicates >= 2^32, cannot be reached through the ABI (no such context
can be created), so no test drives it.
"""
import ctypes as C

import numpy as np
import pytest

import select_law as sl
from ecdna_evo_amd import abi, shard
from support.accept_specs import _final_spec, _passage_spec, _small_spec, _snapshot_spec, _source
from support.gpu import _bytes_of, _run

INF = np.inf


def _tmask(timepoints):
    return sum(1 << t for t in timepoints) if timepoints is not None else 0


def _law(res, source, timepoints=None, **kw):
    records, summ = _source(res, source)
    return sl.select(records, summ, timepoint_mask=_tmask(timepoints), **kw)


def _population(res, source, timepoints=None):
    return sl.population_keys(*_source(res, source), _tmask(timepoints)).shape[1]


def _spread(M, K=32):
    """K ranks: K - 1 spread over 1 .. M (both ends included) and M + 1."""
    return sorted({int(k) for k in np.linspace(1, M, K - 1)})[: K - 1] + [M + 1]


def _nontrivial(want):
    """The preconditions, on the restatement: M >= 2 and at least two selected ks values differ."""
    assert want.population >= 2, want.population
    assert len(set(want.values[0].view(np.uint64).tolist())) >= 2, want.values[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    assert got.population == want.population
    assert got.ranks.dtype == np.uint64 and got.counts_le.dtype == np.uint64 and got.values.dtype == np.float64
    np.testing.assert_array_equal(got.ranks, want.ranks)
    assert got.values.shape == want.values.shape and got.counts_le.shape == want.counts_le.shape
    np.testing.assert_array_equal(_bits(got.values), _bits(want.values))
    np.testing.assert_array_equal(got.counts_le, want.counts_le)


def _check(ctx, res, source, timepoints=None, **kw):
    """ctx.select against the restatement on res = ctx.download(): everything exact."""
    want = _law(res, source, timepoints, **kw)
    got = ctx.select(source, timepoints=timepoints, **kw)
    _same(got, want)
    return want, got


def _accept_agrees(ctx, source, sel, timepoints=None):
    """The contract's consequence: accept with one finite selected value as the only threshold accepts exactly
    counts_le replicates, and with the next smaller double fewer than the rank."""
    assert not np.isnan(sel.values).any()
    at = [(x, j) for x in range(4) for j in range(sel.values.shape[1]) if np.isfinite(sel.values[x, j])]
    assert at
    for below in (False, True):
        cases = [(x, j) for x, j in at if not below or sel.values[x, j] > 0.0]
        for lo in range(0, len(cases), abi.ACCEPT_MAX_THRESHOLDS):
            part = cases[lo:lo + abi.ACCEPT_MAX_THRESHOLDS]
            thr = np.full((len(part), 4), INF)
            for q, (x, j) in enumerate(part):
                thr[q, x] = np.nextafter(sel.values[x, j], -INF) if below else sel.values[x, j]
            accepted = ctx.accept(source, thr, timepoints).counts.sum(axis=1)
            for q, (x, j) in enumerate(part):
                if below:
                    assert int(accepted[q]) < int(sel.ranks[j]), (x, j, sel.values[x, j])
                else:
                    assert int(accepted[q]) == int(sel.counts_le[x, j]), (x, j, sel.values[x, j])


# ------------------------------------------------------------------------------------------- final and sample sources
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["rows", "bins"])
def test_final_and_sample_sources(engine_mod, store):
    """3,000 replicates in 3 sets of 1,000, two workgroups of the digit pass (the second walks a partial round); the
    middle set's replicates all end with ECDNA_REP_ERR_EMPTY, so the population excludes it."""
    ctx, res = _run(engine_mod, _final_spec(store))
    with ctx:
        assert np.all(res.summaries["error"][1000:2000] == abi.REP_ERR_EMPTY)
        for source in (abi.ACCEPT_FINAL, abi.ACCEPT_SAMPLE):
            M = _population(res, source)
            assert M == 2000
            ranks = _spread(M)
            assert len(ranks) == 32 and ranks[0] == 1 and ranks[-2] == M and ranks[-1] == M + 1
            _nontrivial(_law(res, source, ranks=ranks))
            want, got = _check(ctx, res, source, ranks=ranks)
            assert got.population == 2000 and np.all(got.values[:, -1] == INF) and np.all(got.counts_le[:, -1] == M)
            assert np.all(np.diff(got.values[:, :-1], axis=1) >= 0) and np.all(got.counts_le[:, :-1] >= got.ranks[:-1])
            _accept_agrees(ctx, source, got)
            # fractions: the ranks the law derives from M
            want, got = _check(ctx, res, source, fractions=(0.01, 0.5, 1.0))
            assert got.ranks.tolist() == [20, 1000, 2000]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_edge_sizes(engine_mod, n):
    """Lane, wave and workgroup edges, K = 1: the first and the last rank in a call each."""
    ctx, res = _run(engine_mod, _small_spec(n))
    with ctx:
        for source in (abi.ACCEPT_FINAL, abi.ACCEPT_SAMPLE):
            M = _population(res, source)
            if n == 1:
                assert M == 1
            else:
                assert M >= 2
                both = _law(res, source, ranks=[1, M])
                assert _bits(both.values[0])[0] != _bits(both.values[0])[1]  # the two calls' ks values differ
            sels = [_check(ctx, res, source, ranks=[k])[1] for k in (1, M, M + 1)]
            assert np.all(sels[2].values == INF) and np.all(sels[2].counts_le == M)
            for s in sels[:2]:
                _accept_agrees(ctx, source, s)
            _check(ctx, res, source, fractions=[0.5])


# -------------------------------------------------------------------------------------------------- several timepoints
@pytest.mark.gpu
@pytest.mark.parametrize("source", [abi.ACCEPT_SNAPSHOTS, abi.ACCEPT_SNAPSHOT_SAMPLES])
@pytest.mark.parametrize("timepoints", [None, (0, 2)])
def test_snapshot_sources(engine_mod, source, timepoints):
    """[n][S] records, replicate-major, T = 3; a snapshot that was not taken scores ks = 1.0."""
    ctx, res = _run(engine_mod, _snapshot_spec())
    with ctx:
        records, _ = _source(res, source)
        assert records.shape == (192, 3) and (res.snapshots["taken"] == 0).any()
        assert np.all(records["ks"][res.snapshots["taken"] == 0] == 1.0)
        M = _population(res, source, timepoints)
        ranks = _spread(M)
        _nontrivial(_law(res, source, timepoints, ranks=ranks))
        want, got = _check(ctx, res, source, timepoints, ranks=ranks)
        _accept_agrees(ctx, source, got, timepoints)
        if timepoints is not None:  # the middle snapshot decides some order statistic
            assert (_bits(want.values) != _bits(_law(res, source, ranks=ranks).values)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("source", [abi.ACCEPT_PASSAGES, abi.ACCEPT_PASSAGE_SAMPLES])
@pytest.mark.parametrize("timepoints", [None, (0, 1)])
def test_passage_sources(engine_mod, source, timepoints):
    """[G][n] records, phase-major, and one error word per phase: a replicate that errs only in phase 2 belongs to the
    population of phases (0, 1). Extinct phases give ks exactly 1.0 for many replicates: ties on the boundary."""
    ctx, res = _run(engine_mod, _passage_spec())
    with ctx:
        err = res.passages.summaries["error"]  # [G][n]
        only_last = (err[0] == 0) & (err[1] == 0) & (err[2] != 0)
        assert only_last.any() and (err[1] != 0).any() and (err.sum(axis=0) == 0).any()
        M = _population(res, source, timepoints)
        all_free = int((err == 0).all(axis=0).sum())
        assert M == (all_free if timepoints is None else all_free + int(only_last.sum()))
        ranks = sorted(set(_spread(M, 31)[:-1]) | {M - 1}) + [M + 1]  # (M - 1: below the top of a tie at ks = 1.0)
        want = _law(res, source, timepoints, ranks=ranks)
        _nontrivial(want)
        assert (want.counts_le[0][:-1] > want.ranks[:-1]).any()  # a tie is present among the selected ks ranks
        want, got = _check(ctx, res, source, timepoints, ranks=ranks)
        _accept_agrees(ctx, source, got, timepoints)
        _check(ctx, res, source, timepoints, fractions=(0.01, 0.5, 1.0))


# ----------------------------------------------------------------------------------------------------- chunks, shards


@pytest.mark.gpu
def test_two_interleaved_shards_walk_to_the_whole_runs_result(engine_mod):
    ctx, res = _run(engine_mod, _final_spec("bins"))
    with ctx:
        ranks = _spread(_population(res, abi.ACCEPT_FINAL))
        _nontrivial(_law(res, abi.ACCEPT_FINAL, ranks=ranks))
        _, whole = _check(ctx, res, abi.ACCEPT_FINAL, ranks=ranks)
    parts = [_run(engine_mod, _final_spec("bins", first_replicate=g, replicate_stride=2, n_replicates=1500))
             for g in range(2)]
    try:
        for kw in (dict(ranks=ranks), dict(fractions=(0.01, 0.5, 1.0))):
            walk = shard.SelectWalk(len(next(iter(kw.values()))), **kw)
            for p in range(8):
                hists = [c.select_digits(abi.ACCEPT_FINAL, p, walk.prefixes) for c, _ in parts]
                assert all(h.shape == (4, len(walk.prefixes[0]), 256) and h.dtype == np.uint64 for h in hists)
                if p == 0:  # each shard's rows sum to its own M
                    for h, (_, r) in zip(hists, parts):
                        assert np.all(h.sum(axis=2) == _population(r, abi.ACCEPT_FINAL))
                walk.feed(hists[0] + hists[1])
            got = walk.result()
            if "ranks" in kw:
                assert _bytes_of(got) == _bytes_of(whole)
            _same(got, sl.select(*_source(res, abi.ACCEPT_FINAL), **kw))
    finally:
        for c, _ in parts:
            c.close()


@pytest.mark.gpu
def test_sharded_select_over_a_process_group_of_one(engine_mod, tmp_path):
    import torch.distributed as dist

    ctx, res = _run(engine_mod, _snapshot_spec())
    with ctx:
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            got = shard.select(ctx, abi.ACCEPT_SNAPSHOTS, fractions=(0.1, 0.9), timepoints=(0, 2))
        finally:
            dist.destroy_process_group()
        _same(got, _law(res, abi.ACCEPT_SNAPSHOTS, (0, 2), fractions=(0.1, 0.9)))
        assert _bytes_of(got) == _bytes_of(ctx.select(abi.ACCEPT_SNAPSHOTS, fractions=(0.1, 0.9), timepoints=(0, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["final", "snapshots"])
def test_chunked_run_gives_the_same_bytes(engine_mod, kind, monkeypatch):
    spec_of = (lambda: _small_spec(192, "bins")) if kind == "final" else _snapshot_spec
    sources = ((abi.ACCEPT_FINAL, abi.ACCEPT_SAMPLE) if kind == "final"
               else (abi.ACCEPT_SNAPSHOTS, abi.ACCEPT_SNAPSHOT_SAMPLES))
    ctx, res = _run(engine_mod, spec_of())
    with ctx:
        cases = []
        for source in sources:
            ranks = _spread(_population(res, source))
            _nontrivial(_law(res, source, ranks=ranks))
            cases.append((source, ranks, _bytes_of(_check(ctx, res, source, ranks=ranks)[1])))
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "64")
    ctx, res = _run(engine_mod, spec_of())
    with ctx:
        assert ctx.instance()["n_chunks"] == 3
        for source, ranks, whole in cases:
            assert _bytes_of(_check(ctx, res, source, ranks=ranks)[1]) == whole


# ------------------------------------------------------------------------------------------------------ call order
@pytest.mark.gpu
def test_repeated_calls_and_relaunch(engine_mod):
    ctx, res = _run(engine_mod, _final_spec("rows"))
    with ctx:
        L = engine_mod.lib()
        ranks = _spread(_population(res, abi.ACCEPT_FINAL))
        _nontrivial(_law(res, abi.ACCEPT_FINAL, ranks=ranks))
        _, a = _check(ctx, res, abi.ACCEPT_FINAL, ranks=ranks)
        thr = [[float(a.values[0, 10]), INF, INF, INF]]
        acc = ctx.accept(abi.ACCEPT_FINAL, thr, list_capacity=3000)
        assert acc.n_accepted == int(a.counts_le[0, 10])
        # another source and mask in between replaces the cached keys; the first select comes back the same
        _, b = _check(ctx, res, abi.ACCEPT_SAMPLE, ranks=ranks)
        _, a2 = _check(ctx, res, abi.ACCEPT_FINAL, ranks=ranks)
        assert _bytes_of(a2) == _bytes_of(a) != _bytes_of(b)
        again = ctx.download_accept()  # the accept results are still there
        assert again.n_accepted == acc.n_accepted and again.ids.tobytes() == acc.ids.tobytes()
        assert again.mask.tobytes() == acc.mask.tobytes() and again.counts.tobytes() == acc.counts.tobytes()
        # a relaunch drops the keys (and the accept results); select follows the relaunched records
        ctx.launch()
        _, a3 = _check(ctx, ctx.download(), abi.ACCEPT_FINAL, ranks=ranks)
        assert _bytes_of(a3) == _bytes_of(a)
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.E_STATE
    ctx, res2 = _run(engine_mod, _final_spec("rows", seed=8))  # another seed: other records, other order statistics
    with ctx:
        _, c = _check(ctx, res2, abi.ACCEPT_FINAL, ranks=ranks)
        assert c.values.tobytes() != a.values.tobytes()


# ---------------------------------------------------------------------------------------------------------- errors
def _block(ranks=None, fractions=None, **kw):
    d = dict(struct_size=C.sizeof(abi.Select), source=abi.ACCEPT_FINAL)
    keep = []
    if ranks is not None:
        r = np.asarray(ranks, dtype=np.uint64)
        d.setdefault("n_ranks", len(r))
        keep.append(r)
    if fractions is not None:
        f = np.asarray(fractions, dtype=np.float64)
        d.setdefault("n_ranks", len(f))
        keep.append(f)
    d.update(kw)
    s = abi.Select(**d)
    if ranks is not None:
        s.ranks = r.ctypes.data_as(C.POINTER(C.c_uint64))
    if fractions is not None:
        s.fractions = f.ctypes.data_as(C.POINTER(C.c_double))
    s._keep = keep
    return s


def _rc(L, ctx, s):
    pop = C.c_uint64()
    out = np.zeros(4 * 32 * 3, dtype=np.uint64)
    rc = L.ecdna_ssa_ctx_select(ctx.h, C.byref(s) if s is not None else None, C.byref(pop), out.ctypes.data, None, None)
    return rc, L.ecdna_ssa_last_error_message().decode()


def _rc_digits(L, ctx, source=abi.ACCEPT_FINAL, tmask=0, pass_=0, K=1, prefixes=True, hist=True):
    pre = np.zeros((4, 32), dtype=np.uint64)
    out = np.zeros((4, 32, 256), dtype=np.uint64)
    rc = L.ecdna_ssa_ctx_select_digits(ctx.h if ctx is not None else None, source, tmask, pass_, K,
                                       pre.ctypes.data if prefixes else None, out.ctypes.data if hist else None)
    return rc, L.ecdna_ssa_last_error_message().decode()


@pytest.mark.gpu
def test_invalid_arguments(engine_mod):
    L = engine_mod.lib()
    ctx, res = _run(engine_mod, _snapshot_spec())
    with ctx:
        assert _rc(L, ctx, _block([1], source=abi.ACCEPT_SNAPSHOTS))[0] == abi.OK
        assert _rc(L, ctx, _block(fractions=[1.0], source=abi.ACCEPT_SNAPSHOTS, timepoint_mask=0b100))[0] == abi.OK
        bad = [
            ("struct_size", _block([1], struct_size=C.sizeof(abi.Select) - 8)),
            ("struct_size", _block([1], struct_size=0)),
            ("source", _block([1], source=6)),
            ("n_ranks", _block([1], n_ranks=0)),
            ("n_ranks", _block([1] * 33)),
            ("ranks", _block([1], fractions=[0.5])),  # both
            ("fractions", _block(n_ranks=1)),  # neither
            ("ranks[1]", _block([3, 0])),
            ("fractions[0]", _block(fractions=[0.0])),
            ("fractions[1]", _block(fractions=[0.5, 1.0000000000000002])),
            ("fractions[2]", _block(fractions=[0.5, 1.0, np.nan])),
            ("fractions[0]", _block(fractions=[-0.5])),
            ("timepoint_mask", _block([1], source=abi.ACCEPT_SNAPSHOTS, timepoint_mask=0b1000)),
            ("timepoint_mask", _block([1], source=abi.ACCEPT_FINAL, timepoint_mask=0b10)),
            ("reserved", _block([1], reserved=1)),
        ]
        for field, s in bad:
            rc, msg = _rc(L, ctx, s)
            assert rc == abi.E_INVALID and field in msg, (field, rc, msg)
        rc, msg = _rc(L, ctx, None)
        assert rc == abi.E_INVALID and "select is NULL" in msg
        assert L.ecdna_ssa_ctx_select(None, C.byref(_block([1])), None, None, None, None) == abi.E_INVALID
        assert "ctx is NULL" in L.ecdna_ssa_last_error_message().decode()
        # the shard primitive
        assert _rc_digits(L, ctx, abi.ACCEPT_SNAPSHOTS, 0b101, 7, 32)[0] == abi.OK
        for field, kw in (("pass", dict(pass_=8)), ("n_prefixes", dict(K=0)), ("n_prefixes", dict(K=33)),
                          ("prefixes is NULL", dict(prefixes=False)), ("out_hist is NULL", dict(hist=False)),
                          ("source", dict(source=6)),
                          ("timepoint_mask", dict(source=abi.ACCEPT_SNAPSHOTS, tmask=0b1000))):
            rc, msg = _rc_digits(L, ctx, **{"source": abi.ACCEPT_SNAPSHOTS, **kw})
            assert rc == abi.E_INVALID and field in msg, (field, rc, msg)
        rc, msg = _rc_digits(L, None)
        assert rc == abi.E_INVALID and "ctx is NULL" in msg
        # every output of select may be NULL
        assert L.ecdna_ssa_ctx_select(ctx.h, C.byref(_block([1], source=abi.ACCEPT_SNAPSHOTS)), None, None, None,
                                      None) == abi.OK
        # the Python variants raise before they call the library
        for kw in (dict(), dict(ranks=[1], fractions=[0.5]), dict(ranks=[0]), dict(ranks=[-1]), dict(ranks=[2 ** 64]),
                   dict(fractions=[0.0]), dict(fractions=[1.5]), dict(fractions=[np.nan]), dict(ranks=[1] * 33),
                   dict(ranks=[]), dict(ranks=[1], timepoints=(64,)), dict(ranks=[1], timepoints=())):
            with pytest.raises(ValueError):
                ctx.select(abi.ACCEPT_SNAPSHOTS, **kw)
            with pytest.raises(ValueError):
                shard.select(ctx, abi.ACCEPT_SNAPSHOTS, **kw)
        with pytest.raises(ValueError):
            ctx.select_digits(abi.ACCEPT_SNAPSHOTS, 8, np.zeros((4, 1), dtype=np.uint64))
        with pytest.raises(ValueError):
            ctx.select_digits(abi.ACCEPT_SNAPSHOTS, 0, np.zeros((3, 1), dtype=np.uint64))
        with pytest.raises(engine_mod.EngineError):
            ctx.select(abi.ACCEPT_SNAPSHOTS, ranks=[1], timepoints=(3,))


@pytest.mark.gpu
def test_state_errors(engine_mod):
    L = engine_mod.lib()

    def state(ctx, source, word):
        rc, msg = _rc(L, ctx, _block([1], source=source))
        assert rc == abi.E_STATE and word in msg, (source, rc, msg)
        rc, msg = _rc_digits(L, ctx, source)
        assert rc == abi.E_STATE and word in msg, (source, rc, msg)

    with engine_mod.Context(_small_spec(64)) as ctx:  # final and sample statistics, with a target
        state(ctx, abi.ACCEPT_FINAL, "before launch")
        ctx.launch()
        state(ctx, abi.ACCEPT_SNAPSHOTS, "snapshot_stats")
        state(ctx, abi.ACCEPT_SNAPSHOT_SAMPLES, "snapshot_stats")
        state(ctx, abi.ACCEPT_PASSAGES, "ecdna_ssa_ctx_create_passages")
        state(ctx, abi.ACCEPT_PASSAGE_SAMPLES, "ecdna_ssa_ctx_create_passages")
        assert _rc(L, ctx, _block([1], source=abi.ACCEPT_SAMPLE))[0] == abi.OK
        # a refused call leaves the context usable
        assert _rc(L, ctx, _block([1], reserved=1))[0] == abi.E_INVALID
        assert _rc(L, ctx, _block([1]))[0] == abi.OK
    with engine_mod.Context(_small_spec(64, subsample_cells=0)) as ctx:
        ctx.launch()
        state(ctx, abi.ACCEPT_SAMPLE, "subsample_cells")
        assert _rc(L, ctx, _block([1]))[0] == abi.OK
    with engine_mod.Context(_small_spec(64, flags=abi.FLAG_EVENT_HASH, subsample_cells=0, stats_target=None)) as ctx:
        ctx.launch()
        state(ctx, abi.ACCEPT_FINAL, "REP_STATS")
    with engine_mod.Context(_small_spec(64, stats_target=None)) as ctx:  # statistics, but no target: all distances 0
        ctx.launch()
        state(ctx, abi.ACCEPT_FINAL, "without a target")
        state(ctx, abi.ACCEPT_SAMPLE, "without a target")
    with engine_mod.Context(_snapshot_spec(snapshot_subsample_cells=0)) as ctx:
        ctx.launch()
        state(ctx, abi.ACCEPT_SNAPSHOT_SAMPLES, "snapshot_subsample_cells")
        state(ctx, abi.ACCEPT_FINAL, "without a target")  # (the snapshots have targets, the end of the run has none)
        assert _rc(L, ctx, _block([1], source=abi.ACCEPT_SNAPSHOTS))[0] == abi.OK
    with engine_mod.Context(_passage_spec(passage_targets=None)) as ctx:
        state(ctx, abi.ACCEPT_PASSAGES, "before launch")
        ctx.launch()
        state(ctx, abi.ACCEPT_PASSAGES, "without a target")
        state(ctx, abi.ACCEPT_SNAPSHOTS, "snapshot_stats")
