"""Select mapping v1 (include/ecdna_ssa.h, ecdna_ssa_ctx_select) restated in plain numpy: exact order statistics of the
four distances among the error-free replicates of downloaded per-replicate statistics. It does not import the engine.

The population is the replicates without an error (summaries[i].error == 0, or, given one summary per timepoint — the
passage sources — error == 0 at every participating timepoint), pooled over the parameter sets; its size is M. The key
of a distance value: -0.0 -> +0.0, any NaN -> the quiet NaN 0x7FF8000000000000, then bits ^ 0x8000000000000000 for a
clear sign bit and ~bits for a set one, so keys order as the numbers do and NaN sorts above +inf. A replicate's key for
a distance is the maximum of its keys over the participating timepoints. value(k) is the number whose key is the k-th
smallest (np.sort), counts_le(k) the number of keys <= it; k > M gives +inf and M. A fraction f in (0, 1] maps to
k = max(1, ceil(f * M)) in f64.
"""
import math

import numpy as np

from accept_law import timepoints_of

FIELDS = ("ks", "mean_rel", "entropy_rel", "frequency_diff")
SIGN = np.uint64(0x8000000000000000)
QUIET_NAN = np.uint64(0x7FF8000000000000)
PLUS_INF = np.uint64(0x7FF0000000000000)


class Selected:
    """population M; ranks [K] u64; values [4][K] f64 and counts_le [4][K] u64 in the order of FIELDS."""

    def __init__(self, population, ranks, values, counts_le):
        self.population = population
        self.ranks = ranks
        self.values = values
        self.counts_le = counts_le


def keys_of(values):
    """The keys (u64) of an array of f64 distance values."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
    b[(b & ~SIGN) > PLUS_INF] = QUIET_NAN
    b[b == SIGN] = 0
    return np.where(b & SIGN != 0, ~b, b ^ SIGN)


def values_of(keys):
    """The numbers the keys stand for (f64)."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).view(np.float64)


def population_keys(records, summaries, timepoint_mask=0):
    """keys [4][M] u64 of the error-free replicates, in replicate order. records: [n] or [n][T] structured array with
    the four distance FIELDS (replicate-major: a passage download [G][n] is passed transposed); summaries: [n] or
    [n][T] structured array with `error`."""
    records = np.asarray(records)
    if records.ndim == 1:
        records = records[:, None]
    n, T = records.shape
    tps = timepoints_of(int(timepoint_mask), T)
    err = np.asarray(summaries["error"])
    ok = (err[:, tps] == 0).all(axis=1) if err.ndim == 2 else err == 0
    out = np.zeros((4, int(ok.sum())), dtype=np.uint64)
    for x, f in enumerate(FIELDS):
        k = keys_of(records[f][ok][:, tps])
        out[x] = k.max(axis=1) if k.size else np.zeros(0, dtype=np.uint64)
    return out


def rank_of_fraction(f, M):
    assert 0.0 < f <= 1.0
    return max(1, int(math.ceil(float(f) * float(M))))


def select_keys(keys, ranks=None, fractions=None):
    """The order statistics of keys [4][M]."""
    assert (ranks is None) != (fractions is None)
    M = keys.shape[1]
    ranks = [int(k) for k in ranks] if ranks is not None else [rank_of_fraction(f, M) for f in fractions]
    assert 1 <= len(ranks) <= 32 and all(k >= 1 for k in ranks)
    K = len(ranks)
    values = np.full((4, K), np.inf, dtype=np.float64)
    counts_le = np.full((4, K), M, dtype=np.uint64)
    for x in range(4):
        s = np.sort(keys[x])
        for j, k in enumerate(ranks):
            if k > M:
                continue
            values[x, j] = values_of(s[k - 1:k])[0]
            counts_le[x, j] = int(np.searchsorted(s, s[k - 1], side="right"))
    return Selected(M, np.array(ranks, dtype=np.uint64), values, counts_le)


def select(records, summaries, ranks=None, fractions=None, timepoint_mask=0):
    return select_keys(population_keys(records, summaries, timepoint_mask), ranks, fractions)


def digit_hist(keys, pass_, prefixes):
    """ecdna_ssa_ctx_select_digits on keys [4][M]: out[x][j][d] counts the keys of distance x whose top 8 * pass_ bits
    equal those of prefixes[x][j] and whose next 8 bits are d."""
    prefixes = np.asarray(prefixes, dtype=np.uint64).reshape(4, -1)
    K = prefixes.shape[1]
    out = np.zeros((4, K, 256), dtype=np.uint64)
    shift = np.uint64(56 - 8 * pass_)
    for x in range(4):
        digit = ((keys[x] >> shift) & np.uint64(255)).astype(np.int64)
        for j in range(K):
            if pass_ == 0:
                match = np.ones(keys.shape[1], dtype=bool)
            else:
                top = np.uint64(64 - 8 * pass_)
                match = (keys[x] >> top) == (prefixes[x, j] >> top)
            out[x, j] = np.bincount(digit[match], minlength=256).astype(np.uint64)
    return out
