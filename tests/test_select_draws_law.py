"""The numpy restatement of thinned select mapping v1 (tests/select_draws_law.py) on synthetic records, without a GPU:
it is select mapping v1 over the pairs (replicate, draw), so D copies of one record set scale the ranks by D, a
replicate with an error is absent on every draw, and a NaN distance sorts above +inf. A walk over the law's own digit
histograms (contract S1's right-hand side) finds the law's order statistics."""
import numpy as np

import select_draws_law as sdl
import select_law as sl
from ecdna_evo_amd import shard

REC = np.dtype([(f, np.float64) for f in sl.FIELDS])
SUMM = np.dtype([("error", np.uint32)])


def _records(rng, n, T=None):
    shape = (n,) if T is None else (n, T)
    r = np.zeros(shape, dtype=REC)
    for f in sl.FIELDS:
        r[f] = np.round(rng.random(shape), 2)  # (two decimals: ties occur)
    return r


def _summaries(n, bad=()):
    s = np.zeros(n, dtype=SUMM)
    s["error"][list(bad)] = 7
    return s


def test_copies_of_one_record_set_scale_the_ranks():
    rng = np.random.default_rng(5)
    n, D = 37, 5
    rec, summ = _records(rng, n), _summaries(n, bad=(3, 20))
    one = sl.select(rec, summ, ranks=list(range(1, 33)))
    ranks = [int(k) for k in one.ranks]
    many = sdl.select([rec] * D, summ, ranks=[(k - 1) * D + 1 for k in ranks])
    assert many.population == one.population * D == (n - 2) * D
    np.testing.assert_array_equal(many.values.view(np.uint64), one.values.view(np.uint64))
    np.testing.assert_array_equal(many.counts_le, one.counts_le * np.uint64(D))
    # the last of a value's D copies is still that value; one further is the next
    top = sdl.select([rec] * D, summ, ranks=[k * D for k in ranks])
    np.testing.assert_array_equal(top.values.view(np.uint64), one.values.view(np.uint64))
    # fractions cut the same place whatever D
    f = (0.02, 0.25, 0.5, 1.0)
    np.testing.assert_array_equal(sdl.select([rec] * D, summ, fractions=f).values.view(np.uint64),
                                  sl.select(rec, summ, fractions=f).values.view(np.uint64))


def test_a_replicate_with_an_error_is_absent_on_every_draw():
    rng = np.random.default_rng(6)
    n, D = 20, 4
    per_draw = [_records(rng, n) for _ in range(D)]
    for r in per_draw:  # the largest distances by far, were they counted
        for f in sl.FIELDS:
            r[f][[2, 11]] = 50.0
    summ = _summaries(n, bad=(2, 11))
    got = sdl.select(per_draw, summ, ranks=[1, (n - 2) * D, (n - 2) * D + 1])
    assert got.population == (n - 2) * D
    assert np.all(got.values[:, 1] <= 1.0) and np.all(np.isinf(got.values[:, 2]))
    np.testing.assert_array_equal(got.counts_le[:, 2], np.full(4, (n - 2) * D, dtype=np.uint64))
    hist = sdl.digit_hist(per_draw, summ, 0, np.zeros((4, 1), dtype=np.uint64))
    assert np.all(hist.sum(axis=2) == (n - 2) * D)
    # per participating phase: an error in phase 1 only counts when phase 1 takes part
    per_draw2 = [_records(rng, n, 2) for _ in range(D)]
    summ2 = np.zeros((n, 2), dtype=SUMM)
    summ2["error"][[4, 5, 6], 1] = 1
    assert sdl.population_keys(per_draw2, summ2, 0).shape == (4, (n - 3) * D)
    assert sdl.population_keys(per_draw2, summ2, 0b01).shape == (4, n * D)
    assert sdl.population_keys(per_draw2, summ2, 0b10).shape == (4, (n - 3) * D)


def test_a_nan_distance_sorts_above_plus_inf():
    rng = np.random.default_rng(7)
    n, D = 9, 3
    per_draw = [_records(rng, n) for _ in range(D)]
    per_draw[1]["ks"][4] = np.nan
    per_draw[2]["ks"][0] = np.inf
    per_draw[0]["mean_rel"][1] = -0.0
    got = sdl.select(per_draw, _summaries(n), ranks=[n * D - 1, n * D])
    assert np.isinf(got.values[0, 0]) and np.isnan(got.values[0, 1])
    assert got.counts_le[0, 0] == n * D - 1 and got.counts_le[0, 1] == n * D
    assert got.values[1, 1] <= 1.0 and sl.keys_of(np.array([-0.0]))[0] == sl.keys_of(np.array([0.0]))[0]
    # the key of a timepoint maximum: one NaN timepoint makes the pair's key NaN's
    two = [_records(rng, n, 2) for _ in range(D)]
    two[0]["ks"][3, 1] = np.nan
    keys = sdl.population_keys(two, _summaries(n))
    assert (keys[0] == sl.keys_of(np.array([np.nan]))[0]).sum() == 1


def test_the_walk_over_the_laws_digit_histograms_finds_the_laws_statistics():
    rng = np.random.default_rng(8)
    n, D = 41, 6
    per_draw = [_records(rng, n) for _ in range(D)]
    summ = _summaries(n, bad=(0,))
    f = (0.02, 0.3, 0.77, 1.0)
    want = sdl.select(per_draw, summ, fractions=f)
    walk = shard.SelectWalk(len(f), fractions=f)
    for p in range(shard.SelectWalk.PASSES):
        walk.feed(sdl.digit_hist(per_draw, summ, p, walk.prefixes))
    got = walk.result()
    assert got.population == want.population == (n - 1) * D
    np.testing.assert_array_equal(got.ranks, want.ranks)
    np.testing.assert_array_equal(got.values.view(np.uint64), want.values.view(np.uint64))
    np.testing.assert_array_equal(got.counts_le, want.counts_le)
