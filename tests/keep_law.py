"""TEST INFRASTRUCTURE ONLY — numpy restatement of keep mapping v1 (include/ecdna_ssa.h) on top of
tests/subsample_law.py and oracle/abc_stats.py, written from the text of the mapping and not from the kernels.

Replicate r's kept sample is the sample subsample mapping v1 defines for m = keep_cells on its end-of-run population:
its header holds the sample's N- and N+ cell counts, its cells the N+ cells' true copy numbers in ascending order. A
sample the guard ended keeps the header {0xffffffff, 0xffffffff}. A rescored record is the ecdna_rep_stats_t of the kept
sample (all zero under the guard); the pooled histogram of a threshold row sums, per parameter set, the kept samples'
clipped histograms of the replicates whose mask bit is set.
"""
import numpy as np

import abc_stats
import subsample_law as sl

GUARD = 0xFFFFFFFF
ZERO_RECORD = dict(cells=0, mean=0.0, entropy=0.0, frequency=0.0, ks=0.0, mean_rel=0.0, entropy_rel=0.0,
                   frequency_diff=0.0)


def kept(nminus, row, m, seed, rid):
    """((n-, n+), the N+ cells' true copy numbers ascending) of replicate rid's kept sample of m cells; the guard:
    ((GUARD, GUARD), no cells)."""
    s = sl.sample_cells(nminus, row, m, seed, rid)
    if s is None:
        return (GUARD, GUARD), np.zeros(0, dtype=np.int64)
    cells = np.sort(np.asarray(s[1], dtype=np.int64))
    return (int(s[0]), len(cells)), cells


def is_guard(header):
    return int(header[0]) == GUARD and int(header[1]) == GUARD


def kept_hist(header, cells, bins):
    """The kept sample's histogram [bins] (bin 0 = N- cells, true copy numbers clipped at bins - 1; zero under the
    guard)."""
    h = np.zeros(bins, dtype=np.uint64)
    if not is_guard(header):
        c = np.asarray(cells, dtype=np.int64)[: int(header[1])]
        h += np.bincount(np.minimum(c, bins - 1), minlength=bins).astype(np.uint64)
        h[0] += np.uint64(int(header[0]))
    return h


def rescored(header, cells, bins, target):
    """ecdna_rep_stats_t of the kept sample against `target`: abc_stats.rep_stats of its cells, all zero under the
    guard."""
    if is_guard(header):
        return dict(ZERO_RECORD)
    return abc_stats.rep_stats(int(header[0]), np.asarray(cells, dtype=np.int64)[: int(header[1])], bins, target)


def pooled(headers, cells, mask, q, sets, bins, n_sets=None):
    """[n_sets][bins] u64: per parameter set (sets[i]: replicate i's), the sum of the kept samples' histograms of the
    replicates whose mask bit q is set. headers: [n] pairs or a structured array with nminus / nplus; cells: [n][m]."""
    sets = np.asarray(sets, dtype=np.int64)
    n_sets = int(sets.max()) + 1 if n_sets is None else n_sets
    out = np.zeros((n_sets, bins), dtype=np.uint64)
    for i in np.flatnonzero((np.asarray(mask, dtype=np.uint32) >> np.uint32(q)) & np.uint32(1)):
        h = headers[i]
        out[sets[i]] += kept_hist((int(h[0]), int(h[1])), cells[i], bins)
    return out
