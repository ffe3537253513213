"""The cohort of targets of tests/test_gpu_cohort.py, which the keep suite scores its kept samples against."""
import numpy as np

from support.subsample_specs import BINS

# a shared size (64 twice), m = 1, the complement (1500 of up to 2,000), the whole population (4096), a 64-draw batch edge
SAMPLE_CELLS = (64, 1500, 1, 64, 4096, 65)
P = len(SAMPLE_CELLS)


def _targets(bins=BINS):
    """Six distinct histograms: four random ones, one with mass only in bin 0, one only in the overflow bin."""
    rng = np.random.default_rng(41)
    t = np.zeros((P, bins), dtype=np.uint64)
    for p in range(P):
        t[p, 0] = rng.integers(50, 600)
        t[p, 1:20 + 7 * p] = rng.integers(0, 90, 19 + 7 * p)
        t[p, bins - 1] = p
    t[2] = 0
    t[2, 0] = 17
    t[4] = 0
    t[4, bins - 1] = 5
    assert len({row.tobytes() for row in t}) == P
    return t
