"""TEST INFRASTRUCTURE ONLY — numpy restatement of timepoint keep mapping v1 (include/ecdna_ssa.h) on top
of what exists: tests/snapshot_stats_law.py (the sample at a snapshot), tests/passage_law.py (the founders a phase's
sample leaves) and tests/keep_law.py (the kept format, its records and its pooling). Written from the text of the
mapping and not from the kernels.

The kept sample of (replicate r, timepoint t) is a header (n-, n+) with n- + n+ = min(m, N) and the n+ true copy numbers
in ascending order; the guard keeps (GUARD, GUARD).
 - A snapshot context: the sample that snapshot_subsample_cells = m defines for (r, s) — the population "nminus N- cells,
   then the snapshot row", subsample mapping v1 on stream field (s + 1) << 16 under the run's key. Not taken: (0, 0).
 - A passage context: phase g's sample under seed_g, stream field 0: for g < G - 1 the founders of phase g + 1.
Records lie [T][n]; record [t][i] is the record of kept sample [t][i] against target t. The pooled histograms lie
[T][sets][bins].
"""
import numpy as np

import keep_law as kl
import passage_law as pl
import snapshot_stats_law as ssl

GUARD = kl.GUARD


def kept_snapshot(meta, row, m, seed, rid, s):
    """((n-, n+), cells ascending) of replicate rid's kept sample at snapshot s: meta its record (abi.SNAPSHOT_DTYPE),
    row its snapshot row."""
    nm, cells = ssl.state(meta, row)
    sc = ssl.sample_cells(nm, cells, m, seed, rid, s)
    if sc is None:
        return (GUARD, GUARD), np.zeros(0, dtype=np.int64)
    out = np.sort(np.asarray(sc[1], dtype=np.int64))
    return (int(sc[0]), len(out)), out


def kept_phase(nminus, row, m, seed, g, rid):
    """((n-, n+), cells ascending) of replicate rid's kept sample of phase g, from the phase's final state (nminus, row in
    download order): the founders of phase g + 1. (The guard is unreachable at these sizes: passage_law founds the empty
    population for it, the kept header would be (GUARD, GUARD).)"""
    nm, cells = pl.founders(nminus, row, m, seed, g, rid)
    return (int(nm), len(cells)), cells


def rescored(headers, cells, bins, targets):
    """Records [T][n] (a list of lists of dicts): kept sample [t][i] against targets[t]."""
    return [[kl.rescored((int(h[0]), int(h[1])), c, bins, targets[t]) for h, c in zip(headers[t], cells[t])]
            for t in range(len(headers))]


def pooled(headers, cells, mask, q, sets, bins, n_sets=None):
    """[T][n_sets][bins] u64: keep_law.pooled per timepoint, under one mask."""
    return np.stack([kl.pooled(headers[t], cells[t], mask, q, sets, bins, n_sets) for t in range(len(headers))])
