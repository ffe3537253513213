"""Select mapping v1 without a GPU: the numpy restatement (tests/select_law.py) on hand-made records whose answers are
worked out beside them, and shard.SelectWalk, the rank walk a sharded sweep makes over summed digit histograms, against
the restatement. Every comparison is exact: integers and f64 bit patterns."""
import numpy as np
import pytest

import select_law as sl
from ecdna_evo_amd import shard

REC = np.dtype([(f, "<f8") for f in sl.FIELDS])
SUMM = np.dtype([("error", "<u4")])
INF, NAN = np.inf, np.nan


def _records(ks, other=0.25):
    """[n] or [n][T] records with the given ks and one value for the other three distances."""
    ks = np.asarray(ks, dtype=np.float64)
    r = np.zeros(ks.shape, dtype=REC)
    for f in sl.FIELDS:
        r[f] = other
    r["ks"] = ks
    return r


def _errors(err):
    s = np.zeros(np.shape(err), dtype=SUMM)
    s["error"] = err
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    assert got.population == want.population
    np.testing.assert_array_equal(np.asarray(got.ranks, dtype=np.uint64), want.ranks)
    np.testing.assert_array_equal(_bits(got.values), _bits(want.values))
    np.testing.assert_array_equal(np.asarray(got.counts_le, dtype=np.uint64), want.counts_le)


# ------------------------------------------------------------------------------------------------- the restatement
def test_keys_order_as_the_numbers_do_and_invert():
    edge = np.array([-INF, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0 - 2.0 ** -53, 1.0, np.finfo(np.float64).max, INF, NAN])
    k = sl.keys_of(edge)
    assert k[3] == k[4] == np.uint64(0x8000000000000000)  # -0.0 and +0.0 share a key
    d = np.diff(k.astype(object))
    assert all(x > 0 for x in np.delete(d, 3))
    assert int(k[-1]) == 0xFFF8000000000000  # NaN above +inf, below the 64 ones
    assert sl.keys_of(np.array([-NAN]))[0] == k[-1]  # any NaN is the canonical one
    back = sl.values_of(k)
    np.testing.assert_array_equal(_bits(back[:3]), _bits(edge[:3]))
    np.testing.assert_array_equal(_bits(back[4:-1]), _bits(edge[4:-1]))
    assert _bits(back[3:4])[0] == 0 and _bits(back[-1:])[0] == 0x7FF8000000000000


def test_a_tie_on_the_boundary():
    got = sl.select(_records([0.5, 0.2, 0.1, 0.2, 0.2]), _errors([0] * 5), ranks=[1, 2, 3, 4, 5])
    assert got.population == 5
    assert got.values[0].tolist() == [0.1, 0.2, 0.2, 0.2, 0.5]
    assert got.counts_le[0].tolist() == [1, 4, 4, 4, 5]  # > k on the tie
    assert got.values[1].tolist() == [0.25] * 5 and got.counts_le[1].tolist() == [5] * 5  # all equal: every rank ties


def test_minus_zero_next_to_plus_zero():
    got = sl.select(_records([0.0, -0.0, 1.0]), _errors([0, 0, 0]), ranks=[1, 2, 3])
    assert _bits(got.values[0]).tolist() == [0, 0, _bits([1.0])[0]]  # -0.0 is reported as +0.0
    assert got.counts_le[0].tolist() == [2, 2, 3]


def test_a_nan_at_one_timepoint_dominates_and_inf_sorts_below_it():
    # three replicates, two timepoints: maxima 0.3, NaN (0.1 beside a NaN), +inf
    rec = _records([[0.3, 0.2], [0.1, NAN], [INF, 0.0]])
    got = sl.select(rec, _errors([0, 0, 0]), ranks=[1, 2, 3, 4])
    assert got.values[0][0] == 0.3 and got.values[0][1] == INF and np.isnan(got.values[0][2])
    assert _bits(got.values[0][2:3])[0] == 0x7FF8000000000000
    assert got.values[0][3] == INF and got.counts_le[0].tolist() == [1, 2, 3, 3]  # k = M + 1: +inf and M
    # timepoint 0 alone: 0.1, 0.3, +inf, and no NaN
    got = sl.select(rec, _errors([0, 0, 0]), ranks=[1, 2, 3], timepoint_mask=0b01)
    assert got.values[0].tolist() == [0.1, 0.3, INF]


def test_an_error_in_a_phase_that_does_not_take_part_does_not_exclude():
    rec = _records([[0.1, 0.9, 0.2], [0.4, 0.3, 0.8], [0.6, 0.5, 0.7]])
    err = _errors([[0, 0, 2], [0, 2, 0], [0, 0, 0]])  # one summary per phase: the passage sources
    got = sl.select(rec, err, ranks=[1, 2, 3])
    assert got.population == 1 and got.values[0].tolist() == [0.7, INF, INF] and got.counts_le[0].tolist() == [1, 1, 1]
    got = sl.select(rec, err, ranks=[1, 2, 3], timepoint_mask=0b011)  # phases 0, 1: replicate 0 is back
    assert got.population == 2 and got.values[0].tolist() == [0.6, 0.9, INF]
    got = sl.select(rec, err, ranks=[1, 2, 3], timepoint_mask=0b001)
    assert got.population == 3 and got.values[0].tolist() == [0.1, 0.4, 0.6]
    # one summary per replicate (the other sources): an error excludes whatever takes part
    got = sl.select(rec, _errors([0, 5, 0]), ranks=[1, 2], timepoint_mask=0b001)
    assert got.population == 2 and got.values[0].tolist() == [0.1, 0.6]


def test_first_last_and_past_the_last_rank_and_an_empty_population():
    rec = _records([0.4, 0.1, 0.3])
    got = sl.select(rec, _errors([0, 0, 0]), ranks=[1, 3, 4])
    assert got.values[0].tolist() == [0.1, 0.4, INF] and got.counts_le[0].tolist() == [1, 3, 3]
    got = sl.select(rec, _errors([1, 1, 1]), ranks=[1, 2])
    assert got.population == 0 and np.all(got.values == INF) and np.all(got.counts_le == 0)
    got = sl.select(rec, _errors([1, 1, 1]), fractions=[0.5])
    assert got.ranks.tolist() == [1] and np.all(got.values == INF)
    got = sl.select(rec[:0], _errors([]), ranks=[1])
    assert got.population == 0 and np.all(got.values == INF) and np.all(got.counts_le == 0)


def test_ranks_from_fractions():
    assert sl.rank_of_fraction(1e-9, 1000) == 1  # max(1, ceil(1e-6))
    assert sl.rank_of_fraction(0.5, 1001) == 501 and sl.rank_of_fraction(0.5, 1000) == 500
    assert sl.rank_of_fraction(1.0, 1000) == 1000 and sl.rank_of_fraction(1.0, 0) == 1
    assert sl.rank_of_fraction(0.01, 2000) == 20
    got = sl.select(_records(np.arange(10) / 10.0), _errors([0] * 10), fractions=[1e-9, 0.5, 1.0])
    assert got.ranks.tolist() == [1, 5, 10] and got.values[0].tolist() == [0.0, 0.4, 0.9]


# ------------------------------------------------------------------------------------------------- shard.SelectWalk
def _mixed_records(n=1000, T=3, seed=5):
    """Distances with ties (ks on a grid of 40 values, many exactly 1.0), the edge values, and errors in every phase."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, T), dtype=REC)
    rec["ks"] = np.minimum(1.0, rng.integers(0, 60, (n, T)) / 40.0)
    rec["mean_rel"] = rng.random((n, T)) * 10.0 ** rng.integers(-12, 3, (n, T))
    rec["entropy_rel"] = rng.random((n, T))
    rec["frequency_diff"] = rng.integers(0, 8, (n, T)) / 8.0
    rec["mean_rel"][3, 0] = NAN
    rec["mean_rel"][4, 0] = INF
    rec["entropy_rel"][5, 2] = -0.0
    rec["entropy_rel"][5, :2] = 0.0
    rec["frequency_diff"][6] = 5e-324
    err = np.zeros((n, T), dtype=SUMM)
    err["error"] = np.where(rng.random((n, T)) < 0.1, 2, 0)
    err["error"][3:7] = 0
    return rec, err


def _walk(keys_per_shard, K, **kw):
    walk = shard.SelectWalk(K, **kw)
    for p in range(8):
        prefixes = walk.prefixes
        assert prefixes.shape == (4, K) and prefixes.dtype == np.uint64
        total = sum(sl.digit_hist(keys, p, prefixes) for keys in keys_per_shard)
        if p == 0:
            assert all(int(total[x, j].sum()) == sum(k.shape[1] for k in keys_per_shard)
                       for x in range(4) for j in range(K))
        walk.feed(total)
    return walk.result()


@pytest.mark.parametrize("tmask", [0, 0b101])
def test_select_walk_over_three_uneven_shards(tmask):
    rec, err = _mixed_records()
    keys = sl.population_keys(rec, err, tmask)
    M = keys.shape[1]
    assert 500 < M < 1000
    cuts = (0, 137, 738, 1000)
    shards = [sl.population_keys(rec[a:b], err[a:b], tmask) for a, b in zip(cuts, cuts[1:])]
    assert sum(s.shape[1] for s in shards) == M and len({s.shape[1] for s in shards}) == 3
    ranks = [1, 1, 2, 3, M // 100, M // 10, M // 4, M // 4, M // 2, M // 2 + 1, M - 1, M, M, M + 1, M + 1000, 2 ** 63]
    ranks += [int(k) for k in np.linspace(5, M - 5, 32 - len(ranks))]
    assert len(ranks) == 32
    want = sl.select_keys(keys, ranks=ranks)
    assert np.isnan(want.values[1]).any() and (want.counts_le[0] > want.ranks).any()  # a NaN is selected; ks ties
    _same(_walk(shards, 32, ranks=ranks), want)
    _same(_walk([keys], 32, ranks=ranks), want)  # one shard is the whole run


def test_select_walk_fractions_and_an_empty_population():
    rec, err = _mixed_records()
    keys = sl.population_keys(rec, err)
    fr = [1e-9, 0.5, 1.0]
    want = sl.select_keys(keys, fractions=fr)
    assert want.ranks.tolist() == [1, sl.rank_of_fraction(0.5, keys.shape[1]), keys.shape[1]]
    _same(_walk([keys[:, :100], keys[:, 100:]], 3, fractions=fr), want)
    empty = keys[:, :0]
    got = _walk([empty, empty], 2, ranks=[1, 7])
    assert got.population == 0 and np.all(got.values == INF) and np.all(got.counts_le == 0)
    _same(got, sl.select_keys(empty, ranks=[1, 7]))


def test_select_walk_refuses_bad_arguments():
    for kw in (dict(), dict(ranks=[1], fractions=[0.5]), dict(ranks=[0]), dict(fractions=[0.0]), dict(fractions=[1.5]),
               dict(fractions=[NAN]), dict(ranks=list(range(1, 34)))):
        with pytest.raises(ValueError):
            shard.SelectWalk(len(next(iter(kw.values()), [1])), **kw)
    with pytest.raises(ValueError):
        shard.SelectWalk(2, ranks=[1])
    with pytest.raises(ValueError):
        shard.SelectWalk(1, ranks=[1]).result()  # before its eight passes


class _ShardContext:
    """What shard.select asks of a Context: select_digits, here by the restatement over fixed records."""

    def __init__(self, rec, err):
        self.rec, self.err, self.calls = rec, err, []

    def select_digits(self, source, pass_, prefixes, timepoints=None):
        self.calls.append((source, pass_, timepoints))
        tmask = sum(1 << t for t in timepoints) if timepoints is not None else 0
        return sl.digit_hist(sl.population_keys(self.rec, self.err, tmask), pass_, prefixes)


def test_sharded_select_over_a_process_group_of_one(tmp_path):
    import torch.distributed as dist

    rec, err = _mixed_records()
    ctx = _ShardContext(rec, err)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        got = shard.select(ctx, 4, fractions=[0.01, 0.5, 1.0], timepoints=(0, 2))
        by_rank = shard.select(ctx, 4, ranks=[1, 17, 10 ** 6])
    finally:
        dist.destroy_process_group()
    _same(got, sl.select(rec, err, fractions=[0.01, 0.5, 1.0], timepoint_mask=0b101))
    _same(by_rank, sl.select(rec, err, ranks=[1, 17, 10 ** 6]))
    assert ctx.calls[:8] == [(4, p, (0, 2)) for p in range(8)] and len(ctx.calls) == 16  # one exchange per pass
    with pytest.raises(ValueError):
        shard.select(ctx, 4)
    with pytest.raises(ValueError):
        shard.select(ctx, 4, ranks=[0])
