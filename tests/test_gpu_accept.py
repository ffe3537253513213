"""ABC rejection on the GPU (ecdna_ssa_ctx_accept, acceptance mapping v1; include/ecdna_ssa.h).

Every comparison is exact: the mask, the counts, n_accepted and the ids must equal the numpy restatement
(tests/accept_law.py) applied to the same context's downloaded records, and the listed records must be, byte for byte,
the listed rows of that download.

The thresholds come from the run's own downloaded distances, so no case is trivial by construction: the 10 %, 25 %,
50 %, 75 % and 90 % order statistics of each distance among the error-free replicates (the values themselves: ties on
the boundary occur), one all-inf row and one row with ks = 0. Each case first asserts, on the restatement, that some row
accepts strictly between none and all of the error-free replicates. (With n_replicates = 1 no count lies strictly
between 0 and 1: that case asserts instead that one row accepts the replicate and another rejects it.)

One ECDNA_E_INVALID condition of the header, n_replicates >= 2^32, cannot be reached through the ABI: no context with
that many replicates can be created (ecdna_ssa_ctx_create refuses n_replicates > 2^32 - 1), so no test drives it.
"""
import ctypes as C

import numpy as np
import pytest

import accept_law as al
from ecdna_evo_amd import abi
from support.accept_specs import _final_spec, _passage_spec, _small_spec, _snapshot_spec, _source
from support.gpu import ALL_INF_ROW, _run, _thresholds

INF = np.inf


def _law(ctx, res, source, thr, timepoints=None, list_threshold=0, list_capacity=0):
    records, summ = _source(res, source)
    tmask = sum(1 << t for t in timepoints) if timepoints is not None else 0
    return al.accept(records, summ, int(ctx.params.reps_per_set), ctx.spec.replicate_ids(), thr,
                     int(ctx.params.n_param_sets), tmask, list_threshold, list_capacity)


def _nontrivial_row(want, all_inf_row=ALL_INF_ROW):
    """Precondition, on the restatement: some row accepts strictly between none and all of the error-free replicates
    (those the all-inf row accepts). Returns the such row that accepts most."""
    per_row = want.counts.sum(axis=1)
    free = int(per_row[all_inf_row])
    rows = [q for q in range(len(per_row)) if 0 < int(per_row[q]) < free]
    assert rows, (per_row.tolist(), free)
    return max(rows, key=lambda q: int(per_row[q]))


def _check(ctx, res, source, thr, timepoints=None, list_threshold=0, list_capacity=0, want=None):
    """ctx.accept against the restatement on res = ctx.download(): everything exact."""
    if want is None:
        want = _law(ctx, res, source, thr, timepoints, list_threshold, list_capacity)
    got = ctx.accept(source, thr, timepoints, list_threshold, list_capacity)
    records, _ = _source(res, source)
    assert got.mask.dtype == np.uint32 and got.counts.dtype == np.uint64 and got.ids.dtype == np.uint64
    np.testing.assert_array_equal(got.mask, want.mask)
    np.testing.assert_array_equal(got.counts, want.counts)
    assert got.n_accepted == want.n_accepted
    np.testing.assert_array_equal(got.ids, want.ids)
    assert got.stats.shape == (len(want.index), records.shape[1])
    assert got.stats.tobytes() == np.ascontiguousarray(records[want.index]).tobytes()
    return want, got


# ------------------------------------------------------------------------------------------- final and sample sources
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["rows", "bins"])
def test_final_and_sample_sources(engine_mod, store):
    """3,000 replicates in 3 sets of 1,000: 12 workgroups, so the list's order crosses workgroup boundaries, and the
    set boundaries fall inside waves. The middle set's replicates all end with ECDNA_REP_ERR_EMPTY: its counts are 0
    even under the all-inf row."""
    ctx, res = _run(engine_mod, _final_spec(store))
    with ctx:
        n = ctx.spec.n_replicates
        assert np.all(res.summaries["error"][1000:2000] == abi.REP_ERR_EMPTY)
        assert np.all(res.summaries["error"][:1000] == 0) and np.all(res.summaries["error"][2000:] == 0)
        for source in (abi.ACCEPT_FINAL, abi.ACCEPT_SAMPLE):
            records, summ = _source(res, source)
            thr = _thresholds(records, summ)
            q = _nontrivial_row(_law(ctx, res, source, thr))
            want, got = _check(ctx, res, source, thr)  # no list
            assert got.ids.size == 0 and got.stats.shape == (0, 1)
            assert got.counts[ALL_INF_ROW].tolist() == [1000, 0, 1000] and np.all(got.counts[:, 1] == 0)
            assert np.all(got.mask[1000:2000] == 0)
            # the list: below n_accepted (the first entries, in order; n_accepted whole), and room for everyone
            n_acc = int(want.counts[q].sum())
            assert n_acc > 300  # (several workgroups hold accepted replicates)
            want, got = _check(ctx, res, source, thr, list_threshold=q, list_capacity=n_acc // 2)
            assert got.n_accepted == n_acc and len(got.ids) == n_acc // 2 and np.all(np.diff(got.ids.astype(np.int64)) > 0)
            for cap in (n, n + 77):
                want, got = _check(ctx, res, source, thr, list_threshold=q, list_capacity=cap)
                assert len(got.ids) == n_acc and got.ids[-1] >= 2000
            want, got = _check(ctx, res, source, thr, list_threshold=ALL_INF_ROW, list_capacity=n)
            assert got.n_accepted == 2000 and got.ids.tolist() == list(range(1000)) + list(range(2000, 3000))


@pytest.mark.gpu
def test_list_entries_past_the_capacity_are_not_written(engine_mod):
    """The C call with host buffers larger than the capacity, guard-filled: the entries from the capacity on keep the
    guard, the ones before it are the first accepted replicates, and n_accepted is the whole count."""
    ctx, res = _run(engine_mod, _final_spec("bins"))
    with ctx:
        L = engine_mod.lib()
        records, summ = _source(res, abi.ACCEPT_FINAL)
        thr = _thresholds(records, summ)
        q = _nontrivial_row(_law(ctx, res, abi.ACCEPT_FINAL, thr))
        n_acc = int(_law(ctx, res, abi.ACCEPT_FINAL, thr).counts[q].sum())
        cap, extra = n_acc - 5, 16
        assert cap > 0
        want = _law(ctx, res, abi.ACCEPT_FINAL, thr, None, q, cap)
        ctx.accept_enqueue(abi.ACCEPT_FINAL, thr, list_threshold=q, list_capacity=cap)
        ids = np.full(cap + extra, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        stats = np.frombuffer(bytes([0xA5]) * ((cap + extra) * 64), dtype=abi.STATS_DTYPE).copy()
        n_accepted = C.c_uint64()
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, C.byref(n_accepted), ids.ctypes.data,
                                               stats.ctypes.data) == abi.OK
        assert n_accepted.value == n_acc == want.n_accepted
        np.testing.assert_array_equal(ids[:cap], want.ids)
        assert stats[:cap].tobytes() == np.ascontiguousarray(records[want.index, 0]).tobytes()
        assert np.all(ids[cap:] == 0xA5A5A5A5A5A5A5A5) and stats[cap:].tobytes() == bytes([0xA5]) * (extra * 64)
        # every output pointer may be NULL
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.OK


@pytest.mark.gpu
def test_many_sets_per_wave_with_a_stride(engine_mod):
    """reps_per_set = 7 under first_replicate = 5 and replicate_stride = 3: two or three replicates per set, about 25
    set segments in every wave."""
    rates = [(1.0, 1.0 + 0.004 * s, 0.2, 0.25) for s in range(121)]
    spec = _small_spec(280, rates=rates, reps_per_set=7, first_replicate=5, replicate_stride=3)
    ctx, res = _run(engine_mod, spec)
    with ctx:
        assert ctx.params.n_param_sets == 121 and int(spec.replicate_ids()[-1]) // 7 == 120
        for source in (abi.ACCEPT_FINAL, abi.ACCEPT_SAMPLE):
            records, summ = _source(res, source)
            thr = _thresholds(records, summ)
            q = _nontrivial_row(_law(ctx, res, source, thr))
            want, got = _check(ctx, res, source, thr, list_threshold=q, list_capacity=280)
            assert got.counts.shape == (7, 121) and got.counts[ALL_INF_ROW].max() <= 3
            assert np.all((got.ids - 5) % 3 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65])
def test_edge_sizes(engine_mod, n):
    ctx, res = _run(engine_mod, _small_spec(n))
    with ctx:
        records, summ = _source(res, abi.ACCEPT_FINAL)
        thr = _thresholds(records, summ)
        want = _law(ctx, res, abi.ACCEPT_FINAL, thr, None, ALL_INF_ROW, n)
        if n > 1:
            _nontrivial_row(want)
        else:  # one replicate: accepted by the all-inf row, rejected by the ks = 0 row
            assert want.mask[0] & (1 << ALL_INF_ROW) and not want.mask[0] & (1 << (ALL_INF_ROW + 1))
        _check(ctx, res, abi.ACCEPT_FINAL, thr, list_threshold=ALL_INF_ROW, list_capacity=n, want=want)
        _check(ctx, res, abi.ACCEPT_SAMPLE, _thresholds(*_source(res, abi.ACCEPT_SAMPLE)), list_capacity=1)


@pytest.mark.gpu
def test_one_row_and_thirty_two_rows(engine_mod):
    ctx, res = _run(engine_mod, _small_spec(192))
    with ctx:
        records, summ = _source(res, abi.ACCEPT_FINAL)
        thr = _thresholds(records, summ, np.linspace(0.97, 0.03, 32))[:32]
        thr[0] = INF
        thr[31] = [_thresholds(records, summ)[2][0], INF, INF, INF]  # row 31, bit 31 of the mask: the median ks alone
        want = _law(ctx, res, abi.ACCEPT_FINAL, thr, None, 31, 192)
        _nontrivial_row(want, all_inf_row=0)
        per_row = want.counts.sum(axis=1)
        assert 0 < per_row[31] < per_row[0] and (want.mask >> 31).any()
        _check(ctx, res, abi.ACCEPT_FINAL, thr, list_threshold=31, list_capacity=192, want=want)
        one = _thresholds(records, summ)[2:3]  # Q = 1: the medians
        want = _law(ctx, res, abi.ACCEPT_FINAL, one, None, 0, 192)
        assert 0 < want.n_accepted < int((summ["error"] == 0).sum()) and want.mask.max() == 1
        _check(ctx, res, abi.ACCEPT_FINAL, one, list_capacity=192, want=want)


# -------------------------------------------------------------------------------------------------- several timepoints
@pytest.mark.gpu
@pytest.mark.parametrize("source", [abi.ACCEPT_SNAPSHOTS, abi.ACCEPT_SNAPSHOT_SAMPLES])
@pytest.mark.parametrize("timepoints", [None, (0, 2)])
def test_snapshot_sources(engine_mod, source, timepoints):
    """[n][S] records, replicate-major (a replicate that never reaches a snapshot is scored as empty, ks = 1.0)."""
    ctx, res = _run(engine_mod, _snapshot_spec())
    with ctx:
        assert (res.snapshots["taken"][:, 1] == 1).any()
        records, summ = _source(res, source)
        assert records.shape == (192, 3)
        thr = _thresholds(records, summ)
        thr[0] = [INF, INF, INF, float(np.sort(records["frequency_diff"].ravel())[records.size // 2])]
        q = _nontrivial_row(_law(ctx, res, source, thr, timepoints))
        want, got = _check(ctx, res, source, thr, timepoints, list_threshold=q, list_capacity=50)
        assert got.stats.shape[1] == 3  # all T timepoints are listed, whatever takes part
        if timepoints is not None:  # the middle snapshot decides for somebody
            assert (want.mask != _law(ctx, res, source, thr).mask).any()


@pytest.mark.gpu
@pytest.mark.parametrize("source", [abi.ACCEPT_PASSAGES, abi.ACCEPT_PASSAGE_SAMPLES])
@pytest.mark.parametrize("timepoints", [None, (0, 1)])
def test_passage_sources(engine_mod, source, timepoints):
    """[G][n] records, phase-major. Later phases hold ECDNA_REP_ERR_EMPTY replicates; one that errs only in phase 2 is
    acceptable when phases (0, 1) take part."""
    ctx, res = _run(engine_mod, _passage_spec())
    with ctx:
        err = res.passages.summaries["error"]  # [G][n]
        only_last = (err[0] == 0) & (err[1] == 0) & (err[2] != 0)
        assert only_last.any() and (err[1] != 0).any() and (err.sum(axis=0) == 0).any()
        records, summ = _source(res, source)
        assert records.shape == (192, 3)
        free = (err == 0).all(axis=0)
        thr = _thresholds(records[free], summ[free])
        want = _law(ctx, res, source, thr, timepoints)
        _nontrivial_row(want)
        bit = np.uint32(1 << ALL_INF_ROW)
        if timepoints is None:
            assert not (want.mask[only_last] & bit).any()
        else:
            assert (want.mask[only_last] & bit).all() and not (want.mask[err[1] != 0] & bit).any()
        want, got = _check(ctx, res, source, thr, timepoints, list_threshold=ALL_INF_ROW, list_capacity=192)
        assert got.stats.shape[1] == 3 and got.n_accepted == int((want.mask & bit != 0).sum())
        rec_g_n = res.passages.stats if source == abi.ACCEPT_PASSAGES else res.passages.sample_stats
        assert got.stats.tobytes() == np.ascontiguousarray(rec_g_n[:, want.index].T).tobytes()


# ----------------------------------------------------------------------------------------------------- chunks, shards
def _bytes_of(r):
    return (r.mask.tobytes(), r.counts.tobytes(), r.n_accepted, r.ids.tobytes(), r.stats.tobytes())


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
            thr = _thresholds(*_source(res, source))
            q = _nontrivial_row(_law(ctx, res, source, thr))
            want, got = _check(ctx, res, source, thr, list_threshold=q, list_capacity=100)
            cases.append((source, thr, q, _bytes_of(got)))
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "64")
    ctx, res = _run(engine_mod, spec_of())
    with ctx:
        assert ctx.instance()["n_chunks"] == 3
        for source, thr, q, whole in cases:
            want, got = _check(ctx, res, source, thr, list_threshold=q, list_capacity=100)
            assert _bytes_of(got) == whole


@pytest.mark.gpu
def test_two_interleaved_shards_sum_to_the_whole(engine_mod):
    ctx, res = _run(engine_mod, _final_spec("bins"))
    with ctx:
        thr = _thresholds(*_source(res, abi.ACCEPT_FINAL))
        q = _nontrivial_row(_law(ctx, res, abi.ACCEPT_FINAL, thr))
        _, whole = _check(ctx, res, abi.ACCEPT_FINAL, thr, list_threshold=q, list_capacity=3000)
    counts = np.zeros_like(whole.counts)
    ids = []
    for g in range(2):
        ctx, res = _run(engine_mod, _final_spec("bins", first_replicate=g, replicate_stride=2, n_replicates=1500))
        with ctx:
            _, part = _check(ctx, res, abi.ACCEPT_FINAL, thr, list_threshold=q, list_capacity=3000)
        np.testing.assert_array_equal(part.mask, whole.mask[g::2])
        counts += part.counts
        ids.append(part.ids)
    np.testing.assert_array_equal(counts, whole.counts)
    np.testing.assert_array_equal(np.sort(np.concatenate(ids)), whole.ids)


# ------------------------------------------------------------------------------------------------------ call order
@pytest.mark.gpu
def test_repeated_calls_and_relaunch(engine_mod):
    ctx, res = _run(engine_mod, _final_spec("rows"))
    with ctx:
        L = engine_mod.lib()

        def download_all():
            r = ctx.download()
            return tuple(x.tobytes() for x in (r.summaries, r.hist, r.totals, r.stats, r.sample_stats, r.sample_hist))

        before = download_all()
        thr = _thresholds(*_source(res, abi.ACCEPT_FINAL))
        _nontrivial_row(_law(ctx, res, abi.ACCEPT_FINAL, thr))
        # two calls, different thresholds and shapes, no relaunch: each returns its own results
        _, a = _check(ctx, res, abi.ACCEPT_FINAL, thr[:3], list_threshold=2, list_capacity=3000)
        _, b = _check(ctx, res, abi.ACCEPT_SAMPLE, _thresholds(*_source(res, abi.ACCEPT_SAMPLE)), list_threshold=3,
                      list_capacity=10)
        _, a2 = _check(ctx, res, abi.ACCEPT_FINAL, thr[:3], list_threshold=2, list_capacity=3000)
        assert _bytes_of(a) == _bytes_of(a2) != _bytes_of(b)
        assert download_all() == before  # the context's other outputs are untouched
        # a relaunch invalidates the results until the next accept
        ctx.launch()
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.E_STATE
        assert L.ecdna_ssa_last_error_message()
        with pytest.raises(engine_mod.EngineError):
            ctx.download_accept()
        _, a3 = _check(ctx, res, abi.ACCEPT_FINAL, thr[:3], list_threshold=2, list_capacity=3000)
        assert _bytes_of(a3) == _bytes_of(a) and download_all() == before


# ---------------------------------------------------------------------------------------------------------- errors
def _block(thr, **kw):
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    d = dict(struct_size=C.sizeof(abi.Accept), source=abi.ACCEPT_FINAL, n_thresholds=len(thr))
    d.update(kw)
    a = abi.Accept(**d)
    a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
    a._keep = thr
    return a


def _rc(L, ctx, a):
    rc = L.ecdna_ssa_ctx_accept(ctx.h, C.byref(a) if a is not None else None)
    return rc, L.ecdna_ssa_last_error_message().decode()


@pytest.mark.gpu
def test_invalid_arguments(engine_mod):
    L = engine_mod.lib()
    ctx, res = _run(engine_mod, _snapshot_spec())
    one = [[0.5, 0.5, 0.5, 0.5]]
    with ctx:
        assert _rc(L, ctx, _block(one, source=abi.ACCEPT_SNAPSHOTS))[0] == abi.OK
        bad = [
            ("struct_size", _block(one, struct_size=C.sizeof(abi.Accept) - 8)),
            ("struct_size", _block(one, struct_size=0)),
            ("source", _block(one, source=6)),
            ("n_thresholds", _block(one, n_thresholds=0)),
            ("n_thresholds", _block(one * 33)),
            ("list_threshold", _block(one * 2, list_threshold=2)),
            ("thresholds[0].ks", _block([[-1e-300, 0.5, 0.5, 0.5]])),
            ("thresholds[1].entropy_rel", _block([[0.0, INF, 0.0, INF], [0.5, 0.5, np.nan, 0.5]])),
            ("thresholds[0].frequency_diff", _block([[0.5, 0.5, 0.5, -INF]])),
            ("timepoint_mask", _block(one, source=abi.ACCEPT_SNAPSHOTS, timepoint_mask=0b1000)),
            ("timepoint_mask", _block(one, source=abi.ACCEPT_FINAL, timepoint_mask=0b10)),
            ("reserved", _block(one, reserved=1)),
        ]
        for field, a in bad:
            rc, msg = _rc(L, ctx, a)
            assert rc == abi.E_INVALID and field in msg, (field, rc, msg)
        null_thr = _block(one)
        null_thr.thresholds = C.POINTER(abi.AcceptThreshold)()
        rc, msg = _rc(L, ctx, null_thr)
        assert rc == abi.E_INVALID and "thresholds is NULL" in msg
        rc, msg = _rc(L, ctx, None)
        assert rc == abi.E_INVALID and msg
        assert L.ecdna_ssa_ctx_accept(None, C.byref(_block(one))) == abi.E_INVALID and L.ecdna_ssa_last_error_message()
        assert L.ecdna_ssa_ctx_download_accept(None, None, None, None, None, None) == abi.E_INVALID
        assert L.ecdna_ssa_last_error_message()
        # a refused call leaves the last good results in place
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.OK
        with pytest.raises(ValueError):
            ctx.accept(abi.ACCEPT_SNAPSHOTS, [0.5, 0.5, 0.5])
        with pytest.raises(ValueError):
            ctx.accept(abi.ACCEPT_SNAPSHOTS, one, timepoints=(64,))
        with pytest.raises(engine_mod.EngineError):
            ctx.accept(abi.ACCEPT_SNAPSHOTS, one, timepoints=(3,))


@pytest.mark.gpu
def test_state_errors(engine_mod):
    L = engine_mod.lib()
    one = [[0.5, 0.5, 0.5, 0.5]]

    def state(ctx, source, word):
        rc, msg = _rc(L, ctx, _block(one, source=source))
        assert rc == abi.E_STATE and word in msg, (source, rc, msg)

    with engine_mod.Context(_small_spec(64)) as ctx:  # final and sample statistics, with a target
        state(ctx, abi.ACCEPT_FINAL, "before launch")
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.E_STATE
        assert L.ecdna_ssa_last_error_message()
        ctx.launch()
        assert L.ecdna_ssa_ctx_download_accept(ctx.h, None, None, None, None, None) == abi.E_STATE  # before accept
        assert L.ecdna_ssa_last_error_message()
        state(ctx, abi.ACCEPT_SNAPSHOTS, "snapshot_stats")
        state(ctx, abi.ACCEPT_SNAPSHOT_SAMPLES, "snapshot_stats")
        state(ctx, abi.ACCEPT_PASSAGES, "ecdna_ssa_ctx_create_passages")
        state(ctx, abi.ACCEPT_PASSAGE_SAMPLES, "ecdna_ssa_ctx_create_passages")
        assert _rc(L, ctx, _block(one, source=abi.ACCEPT_SAMPLE))[0] == abi.OK
    with engine_mod.Context(_small_spec(64, subsample_cells=0)) as ctx:
        ctx.launch()
        state(ctx, abi.ACCEPT_SAMPLE, "subsample_cells")
        assert _rc(L, ctx, _block(one))[0] == abi.OK
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
        assert _rc(L, ctx, _block(one, source=abi.ACCEPT_SNAPSHOTS))[0] == abi.OK
    with engine_mod.Context(_snapshot_spec(snapshot_targets=None)) as ctx:
        ctx.launch()
        state(ctx, abi.ACCEPT_SNAPSHOTS, "without a target")
    with engine_mod.Context(_passage_spec(passage_targets=None)) as ctx:
        state(ctx, abi.ACCEPT_PASSAGES, "before launch")
        ctx.launch()
        state(ctx, abi.ACCEPT_PASSAGES, "without a target")
        state(ctx, abi.ACCEPT_SNAPSHOTS, "snapshot_stats")
