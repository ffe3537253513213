"""Thinned select mapping v1 (include/ecdna_ssa.h, ecdna_ssa_ctx_select_draws) restated in plain numpy over per-draw
records: select mapping v1 (tests/select_law.py) over the union, over the draws of a range, of the keys of each draw's
records. It does not import the engine.

per_draw is a list, one entry per draw of the range, of the records that draw's sized rescore gives: [n] or [n][T]
structured arrays with the four distance fields, replicate-major. The population is the pairs (error-free replicate,
draw): M = (error-free replicates) x len(per_draw). A pair's key for a distance is the maximum over the participating
timepoints of the key of that draw's record; a replicate with an error is in no draw's keys.
"""
import numpy as np

import select_law as sl


def population_keys(per_draw, summaries, timepoint_mask=0):
    """keys [4][M] u64: the draws' select_law.population_keys side by side (the order within is of no consequence)."""
    assert len(per_draw) >= 1
    return np.concatenate([sl.population_keys(r, summaries, timepoint_mask) for r in per_draw], axis=1)


def select(per_draw, summaries, ranks=None, fractions=None, timepoint_mask=0):
    return sl.select_keys(population_keys(per_draw, summaries, timepoint_mask), ranks, fractions)


def digit_hist(per_draw, summaries, pass_, prefixes, timepoint_mask=0):
    """ecdna_ssa_ctx_select_draws_digits: contract S1, the sum over the draws of each draw's digit histogram."""
    prefixes = np.asarray(prefixes, dtype=np.uint64).reshape(4, -1)
    out = np.zeros((4, prefixes.shape[1], 256), dtype=np.uint64)
    for r in per_draw:
        out += sl.digit_hist(sl.population_keys(r, summaries, timepoint_mask), pass_, prefixes)
    return out
