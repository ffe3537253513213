"""The ABC-statistics run of tests/test_gpu_subsample_stats.py, on which the cohort and keep suites build, with the
tolerances of its float statistics."""
import numpy as np

from ecdna_evo_amd import abi
from support.gpu import _flags

RTOL, ATOL = 1e-12, 1e-14
FLOATS = ("mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")
STORES = [("rows", 0), ("bins", 32), ("bins", 64), ("bins", 256)]
BINS = 257


def _target(bins):
    rng = np.random.default_rng(5)
    t = np.zeros(bins, np.uint64)
    t[0] = 400
    t[1:40] = rng.integers(0, 90, 39)
    t[bins - 1] = 3
    return t


def _abc_spec(store, kmax, with_target, m, **kw):
    """The ABC-statistics spec of tests/test_gpu_abc_stats.py: its 300-copy cell sits in the large-k row for every K."""
    return abi.RunSpec(seed=4, process=abi.BIRTH_DEATH, rates=((1.0, 1.4, 0.3, 0.3), (1.0, 2.0, 0.5, 0.2)),
                       reps_per_set=300, max_cells=2000, hist_bins=BINS, init={1: 3, 300: 1},
                       stats_target=_target(BINS) if with_target else None, flags=_flags(store), bin_kmax=kmax,
                       subsample_cells=m, **{"n_replicates": 600, **kw})
