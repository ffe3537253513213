"""Every timepoint's sample kept on the GPU, scored and pooled after the sweep (ecdna_ssa_keep_timepoints_t, timepoint
keep mapping v1; include/ecdna_ssa.h), on both kinds of longitudinal context: the snapshots of
tests/test_gpu_snapshot_stats.py (600 replicates, two sets, snapshots at 4, 40, 300, 1000 and 2000 cells, 257 bins, a
300-copy cell) and the growth phases of tests/test_gpu_passages.py (192 replicates, three phases).

Every comparison is exact. The kept samples are compared with the numpy restatement (tests/timepoint_keep_law.py)
applied to the run's own snapshot metadata and rows, or to the oracle chain's phase rows; the rescored records with the
launch-time sample records of the same build, as bytes; accept and select over source 13 with the context's own
snapshot-sample or passage-sample source; the pooled histograms with the restatement on the downloaded kept samples and
mask."""
import numpy as np
import pytest

import timepoint_keep_law as tl
from ecdna_evo_amd import abi
from support.gpu import ALL_INF_ROW, _canon, _launched, _same_accept, _same_select, _source_codes, _thresholds
from support.passage_specs import BINS as PBINS
from support.passage_specs import CASES, G, N, _base, _chain, _passage_spec
from support.passage_specs import SEED as PSEED
from support.passage_specs import _targets as _pas_targets
from support.snapshot_specs import BINS as SBINS
from support.snapshot_specs import SNAPS
from support.snapshot_specs import _spec as _snap_spec
from support.snapshot_specs import _targets as _snap_targets

INF = np.inf
S = len(SNAPS)
SNAP_STORES = [("rows", 0), ("bins", 64), ("refdraws", 0)]
PAS_CASES = [c for c in CASES if c[0] in ("rows-pb-binomial-picks", "bins64-bd-binomial-complement", "rows-bd-whole",
                                          "bins32-extinctions", "bins256-bd-binomial-picks")]
FRACTIONS, RANKS = (0.01, 0.1, 0.5, 1.0), (1, 2, 50, 191, 192, 193)
SOURCE = abi.ACCEPT_RESCORED_TIMEPOINTS


def _canon_t(headers, cells):
    return b"".join(_canon(headers[t], cells[t]) for t in range(headers.shape[0]))


def _thresholds_at(rec, summaries, t):
    """support.gpu._thresholds from the records of timepoint t alone (rec: [T][n]): rows that tell replicates apart
    there, whatever the other timepoints hold (a snapshot that was not taken has ks = 1.0 in every replicate)."""
    return _thresholds(np.ascontiguousarray(rec[t][:, None]), summaries)


def _pairs(headers):
    return np.stack([headers["nminus"], headers["nplus"]], axis=-1).astype(np.int64)


# ---- the two kinds of context, behind one face: a spec with the block of m cells (None: no block) and `targets`
# ([T][bins]; None: the suite's own), its launch-time sample records as [T][n], its per-timepoint sample histogram, and
# its own acceptance source ----

class Snapshots:
    T, n, rps, bins, source = S, 600, 300, SBINS, abi.ACCEPT_SNAPSHOT_SAMPLES

    def __init__(self, store="rows", kmax=0, m=64):
        self.store, self.kmax, self.m = store, kmax, m

    def targets(self, which=0):
        t = _snap_targets(SBINS, S)
        return t if which == 0 else np.ascontiguousarray(t[::-1] + np.uint64(1))

    def spec(self, block=True, targets=None, sub=None, **kw):
        """snapshot_subsample_cells = m unless `sub` says otherwise: the launch-time records to compare with."""
        spec = _snap_spec(self.store, self.kmax, True, self.m if sub is None else sub, **kw)
        spec.snapshot_targets = self.targets() if targets is None else targets
        spec.keep_timepoint_cells = self.m if block else None
        return spec

    @staticmethod
    def records(res):
        return np.ascontiguousarray(res.snapshot_sample_stats.T)

    @staticmethod
    def sample_hist(res):
        return res.snapshot_sample_hist

    @staticmethod
    def summaries(res):
        return res.summaries


class Passages:
    T, n, rps, bins, source = G, N, N // 2, PBINS, abi.ACCEPT_PASSAGE_SAMPLES

    def __init__(self, case="rows-pb-binomial-picks"):
        self.case = next(c for c in CASES if c[0] == case)
        self.m = self.case[6]

    def base(self, **kw):
        _, store, kmax, process, seg, rates, _, extra = self.case
        return _base(store, kmax, process, seg, rates, **{**extra, **kw})

    def targets(self, which=0):
        t = _pas_targets()
        return t if which == 0 else np.ascontiguousarray(t[::-1] + np.uint64(1))

    def spec(self, block=True, targets=None, **kw):
        spec = _passage_spec(self.base(**kw), self.m)
        if targets is not None:
            spec.passage_targets = targets
        spec.keep_timepoint_cells = self.m if block else None
        return spec

    @staticmethod
    def records(res):
        return res.passages.sample_stats

    @staticmethod
    def sample_hist(res):
        return res.passages.sample_hist

    @staticmethod
    def summaries(res):
        return np.ascontiguousarray(res.passages.summaries.T)  # [n][G]: every phase's own error word


KINDS = [Snapshots("rows", 0, 64), Snapshots("bins", 64, 700), Passages("rows-pb-binomial-picks"),
         Passages("bins64-bd-binomial-complement")]
KIND_IDS = ["snapshots-rows-64", "snapshots-bins64-700", "passages-rows-pb-picks", "passages-bins64-bd-complement"]


# ---- 1. snapshot samples against the law ----

def _check_snapshot_kept(engine_mod, store, kmax, m):
    spec = Snapshots(store, kmax, m).spec(sub=0)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download()
        headers, cells = ctx.download_kept_timepoints()
    assert headers.dtype == abi.KEPT_DTYPE and headers.shape == (S, 600) and cells.shape == (S, 600, m)
    ids = spec.replicate_ids()
    for i in range(600):
        for s in range(S):
            want_h, want_c = tl.kept_snapshot(res.snapshots[i, s], res.snapshot_rows[i, s], m, spec.seed, int(ids[i]), s)
            got_h = (int(headers[s, i]["nminus"]), int(headers[s, i]["nplus"]))
            assert got_h == want_h, (m, i, s)
            np.testing.assert_array_equal(cells[s, i, :want_h[1]], want_c, err_msg=f"m = {m}, replicate {i}, snapshot {s}")
    # the hard cases occur: snapshots that were not taken (the one at max_cells never is), extinct replicates, and a
    # kept true copy number of 300 above the last bin
    taken = res.snapshots["taken"].T == 1  # [S][n]
    assert not taken[-1].any() and taken[0].all() and 0 < (~taken[1]).sum() < 30
    assert not _pairs(headers)[~taken].any()  # {0, 0}
    pop = (res.snapshots["nminus"] + res.snapshots["nplus"]).T.astype(np.int64) * taken
    np.testing.assert_array_equal(_pairs(headers).sum(axis=-1), np.minimum(pop, m))
    inside = np.arange(m)[None, None, :] < headers["nplus"].astype(np.int64)[:, :, None]
    assert ((cells == 300) & inside).any() and SBINS - 1 < 300
    return pop


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", SNAP_STORES)
@pytest.mark.parametrize("m", [64, 700])
def test_snapshot_samples_against_the_law(engine_mod, store, kmax, m):
    """m = 64: the picks at 300 and 1000 cells, the whole population at 4 and 40; m = 700: the complement at 1000."""
    pop = _check_snapshot_kept(engine_mod, store, kmax, m)
    if m == 64:
        assert (pop[2] == 300).any() and (pop[3] == 1000).any() and np.all(pop[:2] <= 40)
    else:
        assert (pop[3] == 1000).any() and 1000 - m < m < 1000


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 65, 999, 4096])
def test_snapshot_samples_at_the_edges(engine_mod, m):
    """m = 1, the batch edge m = 65, the complement with m' = 1 (999 of 1000), and m = 4096: every population whole."""
    _check_snapshot_kept(engine_mod, "bins", 64, m)


# ---- 2. passage samples against the law ----

@pytest.mark.gpu
@pytest.mark.parametrize("case", PAS_CASES, ids=[c[0] for c in PAS_CASES])
def test_passage_samples_against_the_law(engine_mod, oracle_mod, case):
    name, m = case[0], case[6]
    kind = Passages(name)
    want = _chain(oracle_mod, name, kind.base(), m)
    with _launched(engine_mod, kind.spec()) as ctx:
        res = ctx.download()
        headers, cells = ctx.download_kept_timepoints()
    assert headers.shape == (G, N) and cells.shape == (G, N, m)
    for g in range(G):  # all three phases have a kept sample, the last too
        w = want[g]
        np.testing.assert_array_equal(res.passages.summaries[g]["event_hash"], w["summaries"]["event_hash"])
        for i in range(N):
            want_h, want_c = tl.kept_phase(int(w["summaries"][i]["nminus"]), w["rows"][i], m, PSEED, g, i)
            assert (int(headers[g, i]["nminus"]), int(headers[g, i]["nplus"])) == want_h, (name, g, i)
            np.testing.assert_array_equal(cells[g, i, :want_h[1]], want_c, err_msg=f"{name} phase {g} replicate {i}")
    s = res.passages.summaries
    pop = (s["nminus"] + s["nplus"]).astype(np.int64)
    np.testing.assert_array_equal(_pairs(headers).sum(axis=-1), np.minimum(pop, m))
    assert (pop[G - 1] > 0).any() and _pairs(headers)[G - 1].any()
    if "extinctions" in name:  # an extinct phase, and the phases that never started after it, keep {0, 0}
        dead = pop[0] == 0
        assert dead.any() and not dead.all() and np.all(s["error"][1][dead] == abi.REP_ERR_EMPTY)
        assert not _pairs(headers)[:, dead].any()
    if m == 4096:
        np.testing.assert_array_equal(_pairs(headers).sum(axis=-1), pop)  # the whole population


# ---- 3. rescored records equal the launch-time records, as bytes ----

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_rescored_records_equal_the_launch_time_records(engine_mod, kind):
    X, Y = kind.targets(0), kind.targets(1)
    with _launched(engine_mod, kind.spec(targets=Y)) as other:
        res_y = other.download()
        want_y = kind.records(res_y)
        sel_y = other.select(kind.source, fractions=FRACTIONS)
    with _launched(engine_mod, kind.spec(targets=X)) as ctx:
        res = ctx.download()
        want_x = kind.records(res)
        got = ctx.rescore_timepoints(X)
        assert got.dtype == abi.STATS_DTYPE and got.shape == (kind.T, kind.n)
        assert ctx.accept_timepoints(SOURCE) == kind.T
        for t in range(kind.T):
            for f in abi.STATS_DTYPE.names:  # (named fields first: a failure says which)
                np.testing.assert_array_equal(got[t][f].view(np.uint64), want_x[t][f].view(np.uint64),
                                              err_msg=f"timepoint {t}: {f}")
        assert got.tobytes() == want_x.tobytes()
        assert ctx.download_rescored_timepoints().tobytes() == got.tobytes()
        _same_select(ctx.select(SOURCE, fractions=FRACTIONS), ctx.select(kind.source, fractions=FRACTIONS), "targets X")
        # a second rescore replaces the first: the records of a context created with Y, and the select answers from
        # them (a stale key cache would answer from X's)
        np.testing.assert_array_equal(res.summaries["event_hash"], res_y.summaries["event_hash"])  # the same run
        second = ctx.rescore_timepoints(Y)
        assert second.tobytes() == want_y.tobytes() and second.tobytes() != got.tobytes()
        assert ctx.download_rescored_timepoints().tobytes() == second.tobytes()
        now = ctx.select(SOURCE, fractions=FRACTIONS)
        _same_select(now, sel_y, "targets Y")
        assert now.values.tobytes() != ctx.select(kind.source, fractions=FRACTIONS).values.tobytes()
        assert ctx.rescore_timepoints(X).tobytes() == got.tobytes()


# ---- 4. through accept and select ----

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_through_accept_and_select(engine_mod, kind):
    """Source 13 is the context's own sample source, per timepoint mask and jointly; thresholds from the run's own
    order statistics, so ties on the boundary occur."""
    with _launched(engine_mod, kind.spec()) as ctx:
        res = ctx.download()
        rec = ctx.rescore_timepoints(kind.targets())
        records = np.ascontiguousarray(rec.T)  # [n][T]
        thr = _thresholds(records, kind.summaries(res))
        for tp in [[t] for t in range(kind.T)] + [None, [0, kind.T - 1]]:
            for q, cap in ((0, 0), (2, 50), (ALL_INF_ROW, kind.n)):
                got = ctx.accept(SOURCE, thr, tp, q, cap)
                want = ctx.accept(kind.source, thr, tp, q, cap)
                _same_accept(got, want, f"timepoints {tp}, row {q}")
                assert got.stats.shape == (len(want.ids), kind.T) and got.stats.tobytes() == want.stats.tobytes()
            for kw in (dict(fractions=FRACTIONS), dict(ranks=RANKS)):
                _same_select(ctx.select(SOURCE, timepoints=tp, **kw), ctx.select(kind.source, timepoints=tp, **kw),
                             f"timepoints {tp}")
            hist = [ctx.select_digits(src, 0, np.zeros((4, 1), dtype=np.uint64), tp) for src in (SOURCE, kind.source)]
            np.testing.assert_array_equal(hist[0], hist[1])
        per_row = ctx.accept(SOURCE, thr).counts.sum(axis=1)
        assert 0 < per_row[4] and per_row[0] < per_row[ALL_INF_ROW]


# ---- 5. pooled histograms ----

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS[:3], ids=KIND_IDS[:3])
def test_pooled_accepted_histograms(engine_mod, kind, tmp_path):
    import torch.distributed as dist

    from ecdna_evo_amd import shard

    X = kind.targets()
    spec = kind.spec()
    sets = (spec.replicate_ids() // np.uint64(kind.rps)).astype(np.int64)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download()
        headers, cells = ctx.download_kept_timepoints()
        rec = ctx.rescore_timepoints(X)
        tp = [kind.T // 2]  # (the snapshot at 300 cells; the second phase)
        thr = _thresholds_at(rec, kind.summaries(res), tp[0])
        acc = ctx.accept(SOURCE, thr, tp)
        whole = {}
        for q in (0, 2, ALL_INF_ROW):  # a strict row, a middle row, the all-inf row
            got = ctx.pool_accepted_timepoints(q)
            assert got.dtype == np.uint64 and got.shape == (kind.T, 2, kind.bins)
            np.testing.assert_array_equal(got, tl.pooled(headers, cells, acc.mask, q, sets, kind.bins, 2),
                                          err_msg=f"row {q}")
            whole[q] = got
        assert whole[0].sum() <= whole[2].sum() < whole[ALL_INF_ROW].sum() and whole[2].sum() > 0
        # the all-inf row pools every error-free replicate's samples: the context's own sample histograms
        errors = kind.summaries(res)["error"] != 0
        if isinstance(kind, Passages):
            assert not errors.any()  # the pure-birth case
        if not errors.any():
            np.testing.assert_array_equal(whole[ALL_INF_ROW], kind.sample_hist(res))
        # whatever the source and mask of the accept: the context's own source, every timepoint jointly
        acc1 = ctx.accept(kind.source, _thresholds(np.ascontiguousarray(rec.T), kind.summaries(res)))
        np.testing.assert_array_equal(ctx.pool_accepted_timepoints(1),
                                      tl.pooled(headers, cells, acc1.mask, 1, sets, kind.bins, 2))
        with pytest.raises(engine_mod.EngineError, match="threshold"):
            ctx.pool_accepted_timepoints(len(thr))
        # two interleaved shards' arrays sum to the whole run's
        ctx.accept(SOURCE, thr, tp)
        total = np.zeros((kind.T, 2, kind.bins), dtype=np.uint64)
        for g in range(2):
            with _launched(engine_mod, kind.spec(first_replicate=g, replicate_stride=2,
                                                 n_replicates=kind.n // 2)) as part:
                part.rescore_timepoints(X)
                part.accept(SOURCE, thr, tp)
                total += part.pool_accepted_timepoints(2)
        np.testing.assert_array_equal(total, whole[2])
        # shard.pool_accepted_timepoints over a process group of one
        assert not dist.is_initialized()
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
        try:
            got = shard.pool_accepted_timepoints(ctx, 2)
        finally:
            dist.destroy_process_group()
        np.testing.assert_array_equal(got, whole[2])


# ---- 6. download_kept_timepoints by ids ----

@pytest.mark.gpu
@pytest.mark.parametrize("kind", [KINDS[0], KINDS[3]], ids=[KIND_IDS[0], KIND_IDS[3]])
def test_download_kept_timepoints_by_ids(engine_mod, kind):
    L = engine_mod.lib()
    n, m, T = kind.n, kind.m, kind.T
    with _launched(engine_mod, kind.spec()) as ctx:
        headers, cells = ctx.download_kept_timepoints()
        h5, c5 = ctx.download_kept_timepoints(count=5)
        assert h5.shape == (T, 5) and _canon_t(h5, c5) == _canon_t(headers[:, :5], cells[:, :5])
        out_h, out_c = np.zeros((T, 2), dtype=abi.KEPT_DTYPE), np.zeros((T, 2, m), dtype=np.uint16)
        bad = np.asarray([5, n], dtype=np.uint64)  # an id outside the call; more than the call's replicates
        assert L.ecdna_ssa_ctx_download_kept_timepoints(ctx.h, 2, bad.ctypes.data, out_h.ctypes.data,
                                                        out_c.ctypes.data) == abi.E_INVALID
        assert b"ids[1]" in L.ecdna_ssa_last_error_message()
        assert L.ecdna_ssa_ctx_download_kept_timepoints(ctx.h, n + 1, None, None, None) == abi.E_INVALID
    # the odd shard: the ids in reverse of an accept's list
    with _launched(engine_mod, kind.spec(first_replicate=1, replicate_stride=2, n_replicates=n // 2)) as part:
        res = part.download()
        rec = part.rescore_timepoints(kind.targets())
        tp = kind.T // 2
        acc = part.accept(SOURCE, _thresholds_at(rec, kind.summaries(res), tp), [tp], 3, n)
        assert 1 < len(acc.ids) < n // 2 and np.all(acc.ids % 2 == 1)
        ids = acc.ids[::-1].copy()
        got_h, got_c = part.download_kept_timepoints(ids=ids)
        assert got_h.shape == (T, len(ids)) and got_c.shape == (T, len(ids), m)
        index = ids.astype(np.int64)  # (the whole run's ids are its indices)
        assert _canon_t(got_h, got_c) == _canon_t(headers[:, index], cells[:, index])
        own_h, own_c = part.download_kept_timepoints()
        assert _canon_t(own_h, own_c) == _canon_t(headers[:, 1::2], cells[:, 1::2])
        for bad_id in (2, 0, n + 1):  # off the stride, before the first, past the last
            bad = np.asarray([1, bad_id], dtype=np.uint64)
            assert L.ecdna_ssa_ctx_download_kept_timepoints(part.h, 2, bad.ctypes.data, out_h.ctypes.data,
                                                            out_c.ctypes.data) == abi.E_INVALID, bad_id


# ---- 7. placement independence ----

@pytest.mark.gpu
@pytest.mark.parametrize("kind", [Snapshots("rows", 0, 700), Snapshots("bins", 64, 64), Passages("rows-pb-binomial-picks"),
                                  Passages("bins64-bd-binomial-complement")],
                         ids=["snapshots-rows-700", "snapshots-bins64-64", KIND_IDS[2], KIND_IDS[3]])
def test_placement_independence(engine_mod, kind, monkeypatch):
    """200 replicates in one chunk, as two interleaved shards, and in forced chunks. The snapshot contexts run without
    ECDNA_FLAG_SNAPSHOT_ROWS: their rows are one chunk's scratch."""
    X = kind.targets()
    kw = dict(flags=abi.FLAG_EVENT_HASH) if isinstance(kind, Snapshots) else dict(reps_per_set=100)

    def outputs(ctx):
        headers, cells = ctx.download_kept_timepoints()
        return headers, cells, ctx.rescore_timepoints(X)

    with _launched(engine_mod, kind.spec(n_replicates=200, **kw)) as ctx:
        headers, cells, rec = outputs(ctx)
    assert (headers["nplus"] > 0).sum() > 100
    for g in range(2):
        with _launched(engine_mod, kind.spec(first_replicate=g, replicate_stride=2, n_replicates=100, **kw)) as part:
            ph, pc, prec = outputs(part)
        assert _canon_t(ph, pc) == _canon_t(headers[:, g::2], cells[:, g::2]), g
        assert prec.tobytes() == np.ascontiguousarray(rec[:, g::2]).tobytes(), g
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "101")
    with engine_mod.Context(kind.spec(n_replicates=200, **kw)) as ctx:
        assert ctx.instance()["n_chunks"] == 2 and ctx.row_stride() == 0
        ctx.launch()
        ctx.sync()
        ch, cc, crec = outputs(ctx)
    assert _canon_t(ch, cc) == _canon_t(headers, cells)
    assert crec.tobytes() == rec.tobytes()


# ---- 8. nothing else moves ----

def _raw_calls(L, h, T, n, m, bins):
    """The return codes of the four calls over the kept timepoint samples, with arguments valid on such a context."""
    hists = np.ones((T, bins), dtype=np.uint64)
    rec = np.zeros((T, n), dtype=abi.STATS_DTYPE)
    pool = np.zeros((T, 2, bins), dtype=np.uint64)
    kh, kc = np.zeros((T, n), dtype=abi.KEPT_DTYPE), np.zeros((T, n, max(m, 1)), dtype=np.uint16)
    return (L.ecdna_ssa_ctx_rescore_timepoints(h, hists.ctypes.data),
            L.ecdna_ssa_ctx_download_rescored_timepoints(h, rec.ctypes.data),
            L.ecdna_ssa_ctx_pool_accepted_timepoints(h, 0, pool.ctypes.data),
            L.ecdna_ssa_ctx_download_kept_timepoints(h, n, None, kh.ctypes.data, kc.ctypes.data))


def _downloads(res):
    out = {f: getattr(res, f) for f in ("summaries", "hist", "totals", "stats")}
    if res.passages is not None:
        out.update({"passages." + f: getattr(res.passages, f)
                    for f in ("summaries", "totals", "stats", "sample_stats", "hist", "sample_hist")})
        out.update(sample_stats=res.sample_stats, sample_hist=res.sample_hist)
    else:
        out.update({f: getattr(res, f) for f in ("snapshots", "snapshot_stats", "snapshot_hist",
                                                 "snapshot_sample_stats", "snapshot_sample_hist")})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [KINDS[1], KINDS[3]], ids=[KIND_IDS[1], KIND_IDS[3]])
def test_nothing_else_moves(engine_mod, kind):
    """With the block every other output is that of the same spec without it, and the instance is equal; without it,
    before a launch, before a rescore and after a relaunch the new calls say so."""
    L = engine_mod.lib()
    E, T, n, m, bins = abi.E_STATE, kind.T, kind.n, kind.m, kind.bins
    with engine_mod.Context(kind.spec()) as ctx:
        ins_on = ctx.instance()
        assert _raw_calls(L, ctx.h, T, n, m, bins) == (E, E, E, E)  # before a launch
        assert b"ecdna_ssa_ctx_create_keep_timepoints" in L.ecdna_ssa_last_error_message()
        assert _source_codes(L, ctx.h, SOURCE) == (E, E, E)
        ctx.launch()
        ctx.sync()
        on = ctx.download(want_rows=True)
        assert _source_codes(L, ctx.h, SOURCE) == (E, E, E)  # before a rescore
        assert b"ecdna_ssa_ctx_rescore_timepoints" in L.ecdna_ssa_last_error_message()
        rec_out = np.zeros((T, n), dtype=abi.STATS_DTYPE)
        assert L.ecdna_ssa_ctx_download_rescored_timepoints(ctx.h, rec_out.ctypes.data) == E
        pool = np.zeros((T, 2, bins), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_pool_accepted_timepoints(ctx.h, 0, pool.ctypes.data) == E  # before an accept
        # the calls' own argument checks
        hists = np.ones((T, bins), dtype=np.uint64)
        assert L.ecdna_ssa_ctx_rescore_timepoints(ctx.h, None) == abi.E_INVALID
        hists[1] = 0
        assert L.ecdna_ssa_ctx_rescore_timepoints(ctx.h, hists.ctypes.data) == abi.E_INVALID
        assert b"target_hists[1]" in L.ecdna_ssa_last_error_message()
        rec = ctx.rescore_timepoints(kind.targets())
        # the end-of-run rescore keeps its own records and validity: this context has no keep block
        assert _source_codes(L, ctx.h, abi.ACCEPT_RESCORED) == (E, E, E)
        ctx.accept(SOURCE, [[INF] * 4])
        assert ctx.pool_accepted_timepoints(0).sum() > 0
        assert L.ecdna_ssa_ctx_pool_accepted_timepoints(ctx.h, 1, pool.ctypes.data) == abi.E_INVALID  # threshold >= Q
        assert L.ecdna_ssa_ctx_pool_accepted_timepoints(ctx.h, 0, None) == abi.E_INVALID
        # a relaunch invalidates the records and the acceptance results
        ctx.launch()
        ctx.sync()
        assert L.ecdna_ssa_ctx_download_rescored_timepoints(ctx.h, rec_out.ctypes.data) == E
        assert L.ecdna_ssa_ctx_pool_accepted_timepoints(ctx.h, 0, pool.ctypes.data) == E
        assert _source_codes(L, ctx.h, SOURCE) == (E, E, E)
        assert ctx.rescore_timepoints(kind.targets()).tobytes() == rec.tobytes()  # ... and the same run, the same records
    with engine_mod.Context(kind.spec(block=False)) as ctx:
        assert ctx.keep_timepoints is None and ctx.instance() == ins_on
        ctx.launch()
        ctx.sync()
        off = ctx.download(want_rows=True)
        assert _raw_calls(L, ctx.h, T, n, 0, bins) == (E, E, E, E)  # without the block
        assert b"ecdna_ssa_ctx_create_keep_timepoints" in L.ecdna_ssa_last_error_message()
        assert _source_codes(L, ctx.h, SOURCE) == (E, E, E)
        assert b"ecdna_ssa_ctx_create_keep_timepoints" in L.ecdna_ssa_last_error_message()
        for source in (6, 7, 10, 11, 14):
            assert _source_codes(L, ctx.h, source) == (abi.E_INVALID,) * 3, source
        with pytest.raises(engine_mod.EngineError, match="create_keep_timepoints"):
            ctx.rescore_timepoints(kind.targets())
    a, b = _downloads(on), _downloads(off)
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    for i in range(n):  # (entries past nplus are unspecified)
        np.testing.assert_array_equal(on.row(i), off.row(i))
        for s in range(T if on.snapshot_rows is not None else 0):
            np.testing.assert_array_equal(on.snapshot_row(i, s), off.snapshot_row(i, s))


@pytest.mark.gpu
def test_the_keep_block_beside_a_snapshot_context_stays_independent(engine_mod):
    """Both blocks on one snapshot context: the end-of-run samples and records are those of the keep block alone, and
    each rescore keeps its own records."""
    kind = Snapshots("bins", 64, 64)
    tgt = kind.targets()
    alone = kind.spec(block=False, keep_cells=200)
    with _launched(engine_mod, alone) as ctx:
        want_h, want_c = ctx.download_kept()
        want_rec = ctx.rescore(tgt[:2])
    with _launched(engine_mod, kind.spec(keep_cells=200)) as ctx:
        got_h, got_c = ctx.download_kept()
        assert _canon(got_h, got_c) == _canon(want_h, want_c)
        rec_t = ctx.rescore_timepoints(tgt)
        assert ctx.rescore(tgt[:2]).tobytes() == want_rec.tobytes()
        assert ctx.download_rescored_timepoints().tobytes() == rec_t.tobytes()
        assert ctx.accept_timepoints(abi.ACCEPT_RESCORED) == 2 and ctx.accept_timepoints(SOURCE) == S
        ctx.rescore_timepoints(tgt)
        assert ctx.download_rescored().tobytes() == want_rec.tobytes()


@pytest.mark.gpu
def test_two_blocks_of_different_sizes_share_the_gather_and_the_pool(engine_mod):
    """Both blocks on one snapshot context with samples of 3 and of 5 cells: the gathers by ids and the pooled
    histograms of the two, called in turn, go through the same staging and histogram buffers, and each is its own
    block's — the rows of the whole download, and the sum of the accepted replicates' kept histograms."""
    bins, n, rps = 65, 70, 35  # (70 replicates: more than one wave of them)
    spec = abi.RunSpec(seed=11, process=abi.BIRTH_DEATH, rates=((1.0, 1.4, 0.3, 0.3), (1.0, 2.0, 0.5, 0.2)),
                       reps_per_set=rps, n_replicates=n, max_cells=300, hist_bins=bins, init={1: 3, 40: 1},
                       snapshots=(20, 150), flags=abi.FLAG_REP_STATS | abi.FLAG_EVENT_HASH | abi.FLAG_BIN_STORE,
                       bin_kmax=32, snapshot_stats=True, snapshot_targets=_snap_targets(bins, 2), keep_cells=3,
                       keep_timepoint_cells=5)
    sets = (spec.replicate_ids() // np.uint64(rps)).astype(np.int64)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download()
        h1, c1 = ctx.download_kept()
        ht, ct = ctx.download_kept_timepoints()
        assert c1.shape == (n, 3) and ct.shape == (2, n, 5)
        assert (h1["nplus"] > 0).sum() > n // 2 and (ht["nplus"] > 0).sum() > n // 2
        ids = np.asarray([64, 3, 37], dtype=np.uint64)  # (the call's ids are its indices)
        index = ids.astype(np.int64)
        first = ctx.download_kept(ids=ids)
        timepoints = ctx.download_kept_timepoints(ids=ids)
        third = ctx.download_kept(ids=ids)
        assert first[1].shape == (3, 3) and timepoints[1].shape == (2, 3, 5)
        for got_h, got_c in (first, third):
            assert _canon(got_h, got_c) == _canon(h1[index], c1[index])
        assert _canon_t(*timepoints) == _canon_t(ht[:, index], ct[:, index])
        # one accept, on the snapshot at 150 cells: a proper subset of the replicates
        ks = res.snapshot_stats[:, 1]["ks"]
        acc = ctx.accept(abi.ACCEPT_SNAPSHOTS, [[float(np.median(ks)), INF, INF, INF]], [1])
        assert 0 < acc.n_accepted < n
        pool_first = ctx.pool_accepted(0)
        pool_timepoints = ctx.pool_accepted_timepoints(0)
        pool_third = ctx.pool_accepted(0)
    want = tl.pooled(h1[None], c1[None], acc.mask, 0, sets, bins, 2)[0]
    assert want.sum() > 0
    np.testing.assert_array_equal(pool_first, want)
    np.testing.assert_array_equal(pool_third, pool_first)
    np.testing.assert_array_equal(pool_timepoints, tl.pooled(ht, ct, acc.mask, 0, sets, bins, 2))


# ---- 9. limits ----

@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_limits(engine_mod, store, kmax):
    """The largest table beside the largest histogram: 2,048 bins, m = 4096, 64 pure-birth replicates to 8,200 cells,
    snapshots at 5,000 cells (the complement, m' = 904) and 8,192 (the picks, m' = 4096): one wave per workgroup."""
    bins, m = 2048, 4096
    rng = np.random.default_rng(9)
    targets = rng.integers(0, 50, (2, bins)).astype(np.uint64)
    targets[:, 0] += 1
    store_flag = abi.FLAG_BIN_STORE if store == "bins" else 0
    spec = abi.RunSpec(seed=3, process=abi.PURE_BIRTH, n_replicates=64, max_cells=8200, hist_bins=bins,
                       flags=abi.FLAG_REP_STATS | abi.FLAG_SNAPSHOT_ROWS | abi.FLAG_EVENT_HASH | store_flag,
                       bin_kmax=kmax, snapshots=(5000, 8192), snapshot_stats=True, snapshot_subsample_cells=m,
                       snapshot_targets=targets, keep_timepoint_cells=m)
    with _launched(engine_mod, spec) as ctx:
        res = ctx.download()
        assert np.all(res.snapshots["taken"] == 1) and not (res.summaries["error"] != 0).any()
        assert np.all(res.snapshot_stats["cells"] == (5000, 8192))
        headers, cells = ctx.download_kept_timepoints()
        assert np.all(_pairs(headers).sum(axis=-1) == m)  # headers sum to m
        rec = ctx.rescore_timepoints(targets)
        assert rec.tobytes() == np.ascontiguousarray(res.snapshot_sample_stats.T).tobytes()
        assert np.all(rec["cells"] == m)
        ctx.accept(SOURCE, [[INF] * 4])
        pooled = ctx.pool_accepted_timepoints(0)
    np.testing.assert_array_equal(pooled, res.snapshot_sample_hist)
    assert pooled.sum() == 2 * 64 * m
    ids = spec.replicate_ids()
    for i in (0, 63):  # the law at the limits, on two replicates
        for s in range(2):
            want_h, want_c = tl.kept_snapshot(res.snapshots[i, s], res.snapshot_rows[i, s], m, spec.seed, int(ids[i]), s)
            assert (int(headers[s, i]["nminus"]), int(headers[s, i]["nplus"])) == want_h
            np.testing.assert_array_equal(cells[s, i, :want_h[1]], want_c)
