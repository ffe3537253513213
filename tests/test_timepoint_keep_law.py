"""Timepoint keep mapping v1 restated (tests/timepoint_keep_law.py) against the restatements it stands on, without a
GPU: the kept sample of a snapshot carries the sample snapshot_subsample_cells = m defines there
(tests/snapshot_stats_law.py), the kept sample of a phase the sample the passage pass measures
(tests/subsample_law.py under seed_g), so that rescoring either gives the launch-time record bit for bit. Random small
populations, in the picks, complement and whole-population cases, with cells above the last bin and snapshots that
were not taken."""
import numpy as np

import keep_law as kl
import passage_law as pl
import snapshot_stats_law as ssl
import subsample_law as sl
import timepoint_keep_law as tl

BINS = 12
SEED = 91
FIELDS = ("cells", "mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")
META = np.dtype([("time", "<f8"), ("nminus", "<u8"), ("nplus", "<u8"), ("taken", "<u4"), ("reserved", "<u4")])


def _populations(count):
    """(n-, row, m, rid, t) with N from 0 to ~60 cells, a cell above the last bin in most rows, m on every side of N."""
    rng = np.random.default_rng(321)
    for j in range(count):
        empty = j % 15 == 7
        nminus = 0 if empty else int(rng.integers(0, 25))
        row = rng.integers(1, BINS + 3, 0 if empty else int(rng.integers(0, 40)))
        if len(row) and j % 5:
            row[int(rng.integers(0, len(row)))] = 300
        N = nminus + len(row)
        yield nminus, row, int(rng.integers(1, max(2, N + 8))), 2000 + 7 * j, j % 4


def _bits(rec):
    return [np.float64(rec[f]).view(np.uint64) if f != "cells" else int(rec[f]) for f in FIELDS]


def _check_kept(header, cells, m, N):
    assert header[0] + header[1] == min(m, N) and len(cells) == header[1]  # sizes are min(m, N)
    assert np.all(np.diff(cells) >= 0) and np.all(cells >= 1)  # ascending true copy numbers of N+ cells


def test_kept_snapshot_sample_carries_the_snapshot_sample():
    target = np.arange(1, BINS + 1, dtype=np.uint64)
    seen = {"whole": 0, "picks": 0, "complement": 0, "overflow": 0, "empty": 0, "untaken": 0}
    for nminus, row, m, rid, s in _populations(400):
        taken = rid % 11 != 0
        meta = np.zeros((), dtype=META)
        meta["nminus"], meta["nplus"], meta["taken"] = nminus, len(row), int(taken)
        # (a row longer than nplus: what lies past it is never read)
        stored = np.concatenate([row, np.full(5, 9, dtype=row.dtype)])
        header, cells = tl.kept_snapshot(meta, stored, m, SEED, rid, s)
        N = nminus + len(row) if taken else 0
        _check_kept(header, cells, m, N)
        want_rec, want_hist = ssl.sample(meta, stored, m, SEED, rid, s, BINS, target)
        np.testing.assert_array_equal(kl.kept_hist(header, cells, BINS), want_hist)
        assert _bits(kl.rescored(header, cells, BINS, target)) == _bits(want_rec), (nminus, list(row), m, rid, s)
        if not taken:
            assert header == (0, 0)
            seen["untaken"] += 1
            continue
        seen["empty"] += N == 0
        seen["whole"] += m >= N > 0
        seen["picks"] += m < N and m <= N - m
        seen["complement"] += N - m < m < N
        seen["overflow"] += bool(len(cells)) and int(cells[-1]) == 300
    assert all(v >= 15 for v in seen.values()), seen


def test_the_snapshot_streams_are_apart():
    """The same population sampled at two snapshots, and at the end of the run, gives different draws: the stream field
    is (s + 1) << 16, 0 for the end-of-run sample."""
    row = np.arange(1, 201)
    a = tl.kept_snapshot(dict(taken=1, nminus=50, nplus=200), row, 40, SEED, 5, 0)
    b = tl.kept_snapshot(dict(taken=1, nminus=50, nplus=200), row, 40, SEED, 5, 1)
    c = kl.kept(50, row, 40, SEED, 5)
    assert not (a[0] == b[0] and np.array_equal(a[1], b[1]))
    assert not (a[0] == c[0] and np.array_equal(a[1], c[1]))


def test_kept_phase_sample_carries_the_phase_sample():
    target = np.arange(1, BINS + 1, dtype=np.uint64)
    seen = {"whole": 0, "picks": 0, "complement": 0, "empty": 0}
    for nminus, row, m, rid, g in _populations(300):
        header, cells = tl.kept_phase(nminus, row, m, SEED, g, rid)
        N = nminus + len(row)
        _check_kept(header, cells, m, N)
        key = pl.seed_g(SEED, g)
        np.testing.assert_array_equal(kl.kept_hist(header, cells, BINS), sl.sample_hist(nminus, row, m, key, rid, BINS))
        want = sl.sample_stats(nminus, row, m, key, rid, BINS, target)
        assert _bits(kl.rescored(header, cells, BINS, target)) == _bits(want)
        # ... and it is the founders of the next phase
        nm, f = pl.founders(nminus, row, m, SEED, g, rid)
        assert header == (nm, len(f)) and np.array_equal(cells, f)
        seen["empty"] += N == 0
        seen["whole"] += m >= N > 0
        seen["picks"] += m < N and m <= N - m
        seen["complement"] += N - m < m < N
    assert all(v >= 15 for v in seen.values()), seen


def test_records_and_pools_lie_timepoint_major():
    rng = np.random.default_rng(9)
    T, n, m = 3, 12, 5
    headers = np.zeros((T, n, 2), dtype=np.int64)
    cells = np.zeros((T, n, m), dtype=np.int64)
    for t in range(T):
        for i in range(n):
            nplus = int(rng.integers(0, m + 1))
            headers[t, i] = (int(rng.integers(0, m - nplus + 1)), nplus)
            cells[t, i, :nplus] = np.sort(rng.integers(1, 40, nplus))
    headers[1, 4] = (tl.GUARD, tl.GUARD)
    targets = rng.integers(1, 9, (T, BINS)).astype(np.uint64)
    recs = tl.rescored(headers, cells, BINS, targets)
    assert len(recs) == T and all(len(r) == n for r in recs)
    assert recs[1][4] == kl.ZERO_RECORD
    assert _bits(recs[2][3]) == _bits(kl.rescored(tuple(headers[2, 3]), cells[2, 3], BINS, targets[2]))
    sets = np.arange(n) // 4
    mask = rng.integers(0, 4, n).astype(np.uint32)
    got = tl.pooled(headers, cells, mask, 1, sets, BINS)
    assert got.shape == (T, 3, BINS)
    for t in range(T):
        np.testing.assert_array_equal(got[t], kl.pooled(headers[t], cells[t], mask, 1, sets, BINS))
