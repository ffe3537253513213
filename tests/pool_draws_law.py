"""TEST INFRASTRUCTURE ONLY — numpy restatement of thinned pooling mapping v1 (include/ecdna_ssa.h),
written from the text of the mapping and not from the kernel. It does not import the engine.

The block is thinned acceptance mapping v1's (tests/accept_draws_law.py): slots, each with the kept samples of its
slice, a target, its measured cells m1, the slice's key and snapshot field. Replicate i passes row q on draw d exactly
when that mapping says so. Then, per global parameter set s,
  thinned[slot][s] sums, over the replicates of s and the draws of the range they pass, the clipped histogram of the
      slot's thinned sample on that draw (tests/thin_law.py thinned) — every slot, those the mask leaves out of the
      verdict included; a guard adds nothing;
  kept[slice][s] sums passes[i][q] times the histogram of i's whole kept sample of the slice (tests/keep_law.py
      kept_hist).
"""
import numpy as np

import accept_draws_law as adl
import accept_law as al
import keep_law as kl
import thin_law as tl


def sample_hist(sample, bins):
    """[bins] u64 of a sample (n-, N+ copy numbers): bin 0 holds the N- cells, true copy numbers clip at bins - 1."""
    h = np.zeros(bins, dtype=np.uint64)
    if sample is None:
        return h
    nminus, row = sample
    np.add.at(h, np.minimum(np.asarray(row, dtype=np.int64), bins - 1), np.uint64(1))
    h[0] += np.uint64(nminus)
    return h


def thinned_hists(slots, ids, bins, first_draw, n_draws):
    """[n_slots][n][n_draws][bins] u64: the clipped histogram of every slot's thinned sample of every replicate on every
    draw of the range (all zero under a guard)."""
    out = np.zeros((len(slots), len(ids), n_draws, bins), dtype=np.uint64)
    for t, s in enumerate(slots):
        for i, rid in enumerate(ids):
            h = (int(s.headers[i]["nminus"]), int(s.headers[i]["nplus"]))
            for j in range(n_draws):
                out[t, i, j] = sample_hist(tl.thinned(h, s.cells[i], s.m1, s.key, int(rid), first_draw + j, s.snapshot),
                                           bins)
    return out


def passing(slots, summaries, ids, bins, reps_per_set, n_sets, thresholds, threshold, first_draw, n_draws,
            timepoint_mask=0, per_draw=None):
    """[n][n_draws] bool: replicate i passes row `threshold` on draw first_draw + j. per_draw: the
    accept_draws_law.records(...) of each draw, if the caller has them already."""
    assert 1 <= n_draws and first_draw + n_draws <= 64
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1, 4)
    assert 0 <= threshold < thr.shape[0]
    ok = np.zeros((len(ids), n_draws), dtype=bool)
    for j in range(n_draws):
        rec = per_draw[j] if per_draw is not None else adl.records(slots, ids, bins, first_draw + j)
        mask = al.accept(rec, summaries, reps_per_set, ids, thr, n_sets, timepoint_mask).mask
        ok[:, j] = ((mask >> np.uint32(threshold)) & np.uint32(1)).astype(bool)
    return ok


def pool_draws(slots, slices, summaries, ids, bins, reps_per_set, n_sets, thresholds, threshold, first_draw, n_draws,
               timepoint_mask=0, per_draw=None, hists=None):
    """(thinned [n_slots][n_sets][bins] u64, kept [n_slices][n_sets][bins] u64, passes [n] of the row). slots:
    accept_draws_law.Slot per slot; slices: (headers [n], cells [n][m]) per slice of the store — one for the keep
    store, one per timepoint for the timepoint store. summaries as accept_law.accept takes them. per_draw, hists: the
    records and the thinned_hists(...) of the range, if the caller has them already."""
    ok = passing(slots, summaries, ids, bins, reps_per_set, n_sets, thresholds, threshold, first_draw, n_draws,
                 timepoint_mask, per_draw)
    if hists is None:
        hists = thinned_hists(slots, ids, bins, first_draw, n_draws)
    sets = (np.asarray(ids, dtype=np.uint64) // np.uint64(reps_per_set)).astype(np.int64)
    thinned = np.zeros((len(slots), n_sets, bins), dtype=np.uint64)
    kept = np.zeros((len(slices), n_sets, bins), dtype=np.uint64)
    passes = ok.sum(axis=1)
    for i in np.flatnonzero(passes):
        for t in range(len(slots)):
            thinned[t, sets[i]] += hists[t, i, ok[i]].sum(axis=0, dtype=np.uint64)
        for j, (headers, cells) in enumerate(slices):
            h = (int(headers[i]["nminus"]), int(headers[i]["nplus"]))
            kept[j, sets[i]] += np.uint64(passes[i]) * kl.kept_hist(h, cells[i], bins)
    return thinned, kept, passes
