"""TEST INFRASTRUCTURE ONLY — numpy restatement of passage mapping v1 (include/ecdna_ssa.h), written from
the text of the mapping and not from the kernel.

A run with n_passages = G and passage_cells = m runs G growth phases per replicate. Phase g runs under Philox key
seed_g (seed_0 = seed, else the splitmix64 finaliser of seed + g * 0x9E3779B97F4A7C15). At its end the population (the
n- N- cells, then the N+ row in download order) is sampled by subsample mapping v1 (tests/subsample_law.py) under
seed_g; the sample's N- count and its N+ cells, true copy numbers in ascending order, found phase g + 1.
"""
import numpy as np

import subsample_law as sl

MASK64 = (1 << 64) - 1


def seed_g(seed, g):
    """The key of growth phase g."""
    if g == 0:
        return int(seed) & MASK64
    z = (int(seed) + g * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def founders(nminus, row, m, seed, g, rid):
    """(n-, sorted N+ copy numbers) founding phase g + 1 of replicate rid, from phase g's final state (nminus, row in
    download order). The guard (unreachable) founds the empty population."""
    s = sl.sample_cells(nminus, row, m, seed_g(seed, g), rid)
    if s is None:
        return 0, np.zeros(0, dtype=np.int64)
    return int(s[0]), np.sort(np.asarray(s[1], dtype=np.int64))


def founders_hist(nminus, row, m, seed, g, rid):
    """The founders as an initial histogram {copies: cells} (abi.RunSpec.init / init_per_set): {} when empty."""
    nm, cells = founders(nminus, row, m, seed, g, rid)
    h = {}
    if nm:
        h[0] = nm
    ks, cnt = np.unique(cells, return_counts=True)
    for k, c in zip(ks.tolist(), cnt.tolist()):
        h[int(k)] = int(c)
    return h
