"""Acceptance mapping v1 (include/ecdna_ssa.h, ecdna_ssa_ctx_accept) restated in plain numpy: ABC rejection over
downloaded per-replicate statistics. It does not import the engine.

Replicate i is accepted under threshold row q iff (1) it is error-free — summaries[i].error == 0, or, given one summary
per timepoint (the passage sources), error == 0 at every participating timepoint — and (2) for every participating
timepoint t and each distance x of (ks, mean_rel, entropy_rel, frequency_diff): thr[q].x == +inf or d[i][t].x <=
thr[q].x. A tie passes; a NaN distance fails unless the threshold is +inf.
"""
import numpy as np

FIELDS = ("ks", "mean_rel", "entropy_rel", "frequency_diff")


class Accepted:
    """mask [n] u32 (bit q: accepted under row q); counts [Q][n_sets] u64; n_accepted under the list's row (the whole
    count); index [n_listed]: the call indices i of the first min(n_accepted, list_capacity) accepted replicates in
    ascending order, and ids [n_listed]: their global ids."""

    def __init__(self, mask, counts, n_accepted, index, ids):
        self.mask = mask
        self.counts = counts
        self.n_accepted = n_accepted
        self.index = index
        self.ids = ids


def timepoints_of(timepoint_mask, T):
    """The participating timepoints: the set bits of the mask, or all T when it is 0."""
    if timepoint_mask == 0:
        return list(range(T))
    assert timepoint_mask >> T == 0, "timepoint_mask has bits at or above T"
    return [t for t in range(T) if (timepoint_mask >> t) & 1]


def accept(records, summaries, reps_per_set, ids, thresholds, n_sets, timepoint_mask=0, list_threshold=0,
           list_capacity=0):
    """records: [n] or [n][T] structured array with the four distance FIELDS (replicate-major: a passage download
    [G][n] is passed transposed); summaries: [n] or [n][T] structured array with `error`; ids: [n] global replicate
    ids; thresholds: [Q][4] in the order of FIELDS."""
    records = np.asarray(records)
    if records.ndim == 1:
        records = records[:, None]
    n, T = records.shape
    tps = timepoints_of(int(timepoint_mask), T)
    err = np.asarray(summaries["error"])
    bad = (err[:, tps] != 0).any(axis=1) if err.ndim == 2 else err != 0
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1, 4)
    Q = thr.shape[0]
    assert 1 <= Q <= 32 and list_threshold < Q
    ids = np.asarray(ids, dtype=np.uint64)
    sets = (ids // np.uint64(reps_per_set)).astype(np.int64)
    mask = np.zeros(n, dtype=np.uint32)
    counts = np.zeros((Q, n_sets), dtype=np.uint64)
    for q in range(Q):
        ok = ~bad
        for t in tps:
            for k, f in enumerate(FIELDS):
                if thr[q, k] == np.inf:
                    continue
                with np.errstate(invalid="ignore"):
                    ok &= records[f][:, t] <= thr[q, k]  # (NaN <= x is False)
        mask |= ok.astype(np.uint32) << np.uint32(q)
        counts[q] = np.bincount(sets[ok], minlength=n_sets).astype(np.uint64)
    index = np.nonzero((mask >> np.uint32(list_threshold)) & np.uint32(1))[0]
    n_accepted = int(index.size)
    index = index[: min(n_accepted, int(list_capacity))]
    return Accepted(mask, counts, n_accepted, index, ids[index])
