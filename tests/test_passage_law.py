"""The numpy restatement of passage mapping v1 (tests/passage_law.py) without a GPU: the phase keys against values
worked out here with Python integers, and the founders' law against the exact hypergeometric pmf, with the founders of
two phases independent of each other."""
import numpy as np
from scipy import stats

import passage_law as pl
import subsample_law as sl
from ecdna_evo_amd import abi
from exact_law import chi2_lumped

N_IDS = 1 << 16
# a fixed population of 12 cells: 4 N- cells, then the row in download order; the marked kind is k = 5 (3 cells)
NMINUS, ROW = 4, np.asarray([1, 5, 1, 2, 5, 2, 1, 5], dtype=np.uint16)
MARKED, N_MARKED, N_CELLS = 5, 3, 12


def test_seed_g_is_the_splitmix64_finaliser():
    M = (1 << 64) - 1
    for seed in (0, 1, 26, 42, 2**63 + 12345, M):
        assert pl.seed_g(seed, 0) == seed
        for g in (1, 2, 15):
            z = (seed + g * 0x9E3779B97F4A7C15) % (1 << 64)
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
            want = z ^ (z >> 31)
            assert pl.seed_g(seed, g) == want == abi.passage_seed(seed, g), (seed, g)
    # splitmix64's published first outputs from states 0 and 1 (state += golden ratio, then the finaliser)
    assert pl.seed_g(0, 1) == 0xE220A8397B1DCDAF and pl.seed_g(1, 1) == 0x910A2DEC89025CC1
    keys = {pl.seed_g(7, g) for g in range(16)}
    assert len(keys) == 16


def test_founders_are_the_sorted_sample():
    for m in (1, 5, 6, 9, 11, 12, 40):
        for g in (0, 1):
            nm, cells = pl.founders(NMINUS, ROW, m, 3, g, 77)
            want = sl.sample_cells(NMINUS, ROW, m, pl.seed_g(3, g), 77)
            assert nm == want[0] and cells.tolist() == sorted(int(x) for x in want[1])
            assert nm + len(cells) == min(m, N_CELLS)
            h = pl.founders_hist(NMINUS, ROW, m, 3, g, 77)
            assert h.get(0, 0) == nm and sum(v for k, v in h.items() if k) == len(cells)
    nm, cells = pl.founders(NMINUS, ROW, 12, 3, 1, 5)  # m >= N: everything
    assert nm == NMINUS and cells.tolist() == sorted(ROW.tolist())
    assert pl.founders_hist(0, [], 5, 3, 1, 5) == {}  # nothing to sample


def _marked_counts(m, g):
    return np.asarray([int((pl.founders(NMINUS, ROW, m, 9, g, rid)[1] == MARKED).sum()) for rid in range(N_IDS)])


def test_founders_follow_the_hypergeometric_law_and_phases_are_independent():
    """m = 5 (the picks are the sample) and m = 9 (the complement: m' = 3 cells are left out): the number of marked
    cells among the founders is Hypergeometric(12, 3, m); the counts under seed_0 and seed_1, replicate by replicate,
    fill the product table (a chi-square of the joint table against the product of the two exact pmfs)."""
    for m in (5, 9):
        x0, x1 = _marked_counts(m, 0), _marked_counts(m, 1)
        pmf = stats.hypergeom.pmf(np.arange(N_MARKED + 1), N_CELLS, N_MARKED, m)
        for g, x in ((0, x0), (1, x1)):
            p = chi2_lumped(np.bincount(x, minlength=N_MARKED + 1), pmf * N_IDS, min_expected=5)
            assert p > 1e-6, (m, g, p)
        joint = np.bincount(x0 * (N_MARKED + 1) + x1, minlength=(N_MARKED + 1) ** 2)
        p = chi2_lumped(joint, np.outer(pmf, pmf).ravel() * N_IDS, min_expected=5)
        assert p > 1e-6, (m, "joint", p)
        assert not np.array_equal(x0, x1)
