"""The end-to-end run of tests/test_gpu_sample_states.py on a synthetic final state, which the thinning suites run
again: ids with a high word and a stride, the sample, the keep block and a cohort of two targets."""
import numpy as np

from ecdna_evo_amd import abi

SEED = 2027
RID0, RID_STRIDE = 2**40 + 5, 3


def _target(bins):
    rng = np.random.default_rng(5)
    t = np.zeros(bins, np.uint64)
    t[0] = 400
    t[1:30] = rng.integers(0, 90, 29)
    t[bins - 1] = 3
    return t


E2E_BINS = 33


def _e2e_spec(store, init, **kw):
    """64 replicates under ids with a high word and a stride, the sample, the keep block and a cohort of two targets
    with sample sizes (200, 4096)."""
    t = _target(E2E_BINS)
    flags = abi.FLAG_REP_STATS | (abi.FLAG_BIN_STORE if store == "bins" else 0)
    return abi.RunSpec(seed=SEED, process=abi.BIRTH_DEATH, rates=((1.0, 1.4, 0.3, 0.3),), n_replicates=64,
                       first_replicate=RID0, replicate_stride=RID_STRIDE, hist_bins=E2E_BINS, init=init, flags=flags,
                       bin_kmax=64 if store == "bins" else 0, stats_target=t, subsample_cells=4096, keep_cells=4096,
                       cohort_targets=np.stack([t[::-1].copy(), t]), cohort_sample_cells=(200, 4096), **kw)
