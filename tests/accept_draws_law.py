"""TEST INFRASTRUCTURE ONLY — numpy restatement of thinned acceptance mapping v1 (include/ecdna_ssa.h),
written from the text of the mapping and not from the kernel. It does not import the engine.

A call names acceptance timepoints ("slots"): on the keep store the P targets of the one slice, on the timepoint store
one target per slice. For a draw d, slot t's record is thinning mapping v1's (tests/thin_law.py record) of the slot's
kept sample on sample_cells[t] cells and draw d, under the slot's key and snapshot field. Replicate i passes row q on
draw d iff acceptance mapping v1 (tests/accept_law.py) accepts it on those records; passes[i][q] counts the draws of
first_draw .. first_draw + n_draws - 1 it passes, and sums[q][s] adds passes over the replicates of global set s.
"""
import numpy as np

import accept_law as al
import thin_law as tl

DISTANCES = np.dtype([(f, np.float64) for f in al.FIELDS])


class Slot:
    """One acceptance timepoint: the kept samples it is scored on (headers [n] with nminus / nplus, cells [n][m]), the
    target histogram, the measured cells m1, and the key and snapshot index of the slice (thin_law.phase_key; None: the
    end of the run or a passage phase)."""

    def __init__(self, headers, cells, target, m1, key, snapshot=None):
        self.headers, self.cells, self.target, self.m1, self.key, self.snapshot = headers, cells, target, m1, key, snapshot


def records(slots, ids, bins, d):
    """[n][T] distances of every replicate's thinned sample of every slot on draw d."""
    out = np.zeros((len(ids), len(slots)), dtype=DISTANCES)
    for t, s in enumerate(slots):
        for i, rid in enumerate(ids):
            h = (int(s.headers[i]["nminus"]), int(s.headers[i]["nplus"]))
            r = tl.record(h, s.cells[i], s.m1, s.key, int(rid), bins, s.target, d, s.snapshot)
            for f in al.FIELDS:
                out[i, t][f] = r[f]
    return out


def accept_draws(slots, summaries, ids, bins, reps_per_set, n_sets, thresholds, first_draw, n_draws, timepoint_mask=0,
                 per_draw=None):
    """(passes [n][Q] u8, sums [Q][n_sets] u64). summaries: [n] or [n][T] with `error`, as accept_law.accept takes them.
    per_draw: the records(...) of each draw, if the caller has them already."""
    assert 1 <= n_draws and first_draw + n_draws <= 64
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1, 4)
    Q = thr.shape[0]
    passes = np.zeros((len(ids), Q), dtype=np.uint8)
    for j, d in enumerate(range(first_draw, first_draw + n_draws)):
        rec = per_draw[j] if per_draw is not None else records(slots, ids, bins, d)
        mask = al.accept(rec, summaries, reps_per_set, ids, thr, n_sets, timepoint_mask).mask
        for q in range(Q):
            passes[:, q] += ((mask >> np.uint32(q)) & np.uint32(1)).astype(np.uint8)
    sets = (np.asarray(ids, dtype=np.uint64) // np.uint64(reps_per_set)).astype(np.int64)
    sums = np.zeros((Q, n_sets), dtype=np.uint64)
    for q in range(Q):
        sums[q] = np.bincount(sets, weights=passes[:, q].astype(np.float64), minlength=n_sets).astype(np.uint64)
    return passes, sums
