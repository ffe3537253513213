"""Keep mapping v1 restated (tests/keep_law.py) against subsample mapping v1's restatement (tests/subsample_law.py),
without a GPU: a kept sample — header and ascending true copy numbers — carries everything the sample's record and
histogram are made of, so that rescoring it gives the launch-time sample record bit for bit. Random small populations,
in the picks, complement and whole-population cases, each with a cell above the last bin."""
import numpy as np

import keep_law as kl
import subsample_law as sl

BINS = 12
SEED = 77
FIELDS = ("cells", "mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")


def _populations(count):
    """(n-, row, m, rid) with N from 0 to ~60 cells, one cell above the last bin in most rows, m on every side of N."""
    rng = np.random.default_rng(123)
    for j in range(count):
        empty = j % 15 == 7  # an extinct replicate
        nminus = 0 if empty else int(rng.integers(0, 25))
        row = rng.integers(1, BINS + 3, 0 if empty else int(rng.integers(0, 40)))
        if len(row) and j % 5:
            row[int(rng.integers(0, len(row)))] = 300  # far above the last bin: the true copy number is kept
        N = nminus + len(row)
        m = int(rng.integers(1, max(2, N + 8)))
        yield nminus, row, m, 1000 + 3 * j


def _bits(rec):
    return [np.float64(rec[f]).view(np.uint64) if f != "cells" else int(rec[f]) for f in FIELDS]


def test_kept_sample_carries_the_sample():
    target = np.arange(1, BINS + 1, dtype=np.uint64)
    seen = {"whole": 0, "picks": 0, "complement": 0, "overflow": 0, "empty": 0}
    for nminus, row, m, rid in _populations(400):
        N = nminus + len(row)
        header, cells = kl.kept(nminus, row, m, SEED, rid)
        assert header[0] + header[1] == min(m, N) and len(cells) == header[1]
        assert np.all(np.diff(cells) >= 0) and np.all(cells >= 1)
        np.testing.assert_array_equal(kl.kept_hist(header, cells, BINS), sl.sample_hist(nminus, row, m, SEED, rid, BINS))
        for tgt in (target, None):
            want = sl.sample_stats(nminus, row, m, SEED, rid, BINS, tgt)
            assert _bits(kl.rescored(header, cells, BINS, tgt)) == _bits(want), (nminus, list(row), m, rid)
        seen["empty"] += N == 0
        seen["whole"] += m >= N > 0
        seen["picks"] += m < N and m <= N - m
        seen["complement"] += N - m < m < N
        seen["overflow"] += bool(len(cells)) and int(cells[-1]) == 300
        # cells past nplus are unspecified: a padded row rescored the same
        padded = np.concatenate([cells, np.full(3, 9, dtype=np.int64)])
        assert _bits(kl.rescored(header, padded, BINS, target)) == _bits(kl.rescored(header, cells, BINS, target))
    assert all(v >= 20 for v in seen.values()), seen  # no case is silently absent


def test_the_guard_header_is_the_all_zero_record():
    header = (kl.GUARD, kl.GUARD)
    assert kl.is_guard(header) and not kl.is_guard((kl.GUARD, 0)) and not kl.is_guard((0, 0))
    rec = kl.rescored(header, np.zeros(0, dtype=np.int64), BINS, np.ones(BINS, dtype=np.uint64))
    assert rec == kl.ZERO_RECORD
    assert not kl.kept_hist(header, np.zeros(0, dtype=np.int64), BINS).any()
    # the empty sample is not the guard: ks = 1.0 with a target
    assert kl.rescored((0, 0), np.zeros(0, dtype=np.int64), BINS, np.ones(BINS, dtype=np.uint64))["ks"] == 1.0


def test_pooled_sums_the_accepted_samples_per_set():
    rng = np.random.default_rng(5)
    n, m = 40, 6
    headers = np.zeros((n, 2), dtype=np.int64)
    cells = np.zeros((n, m), dtype=np.int64)
    for i in range(n):
        nplus = int(rng.integers(0, m + 1))
        headers[i] = (int(rng.integers(0, m - nplus + 1)), nplus)
        cells[i, :nplus] = np.sort(rng.integers(1, 40, nplus))
        cells[i, nplus:] = 7  # unspecified entries must not be counted
    headers[3] = (kl.GUARD, kl.GUARD)
    sets = np.arange(n) // 10
    mask = rng.integers(0, 8, n).astype(np.uint32)
    mask[3] |= 2
    for q in range(3):
        got = kl.pooled(headers, cells, mask, q, sets, BINS)
        assert got.shape == (4, BINS)
        acc = [i for i in range(n) if (mask[i] >> q) & 1 and i != 3]
        assert got.sum() == sum(int(headers[i].sum()) for i in acc)
        for s in range(4):
            want = sum((kl.kept_hist(headers[i], cells[i], BINS) for i in acc if sets[i] == s),
                       np.zeros(BINS, dtype=np.uint64))
            np.testing.assert_array_equal(got[s], want)
    assert not kl.pooled(headers, cells, np.zeros(n, dtype=np.uint32), 0, sets, BINS).any()
