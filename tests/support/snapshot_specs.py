"""The run of tests/test_gpu_snapshot_stats.py, which the timepoint keep suite runs again with the timepoint keep
block."""
import numpy as np

from ecdna_evo_amd import abi

BINS = 257
SNAPS = (4, 40, 300, 1000, 2000)


def _targets(bins, n):
    """One target per snapshot, each its own."""
    rng = np.random.default_rng(5)
    t = np.zeros((n, bins), np.uint64)
    for s in range(n):
        t[s, 0] = 400 - 50 * s
        t[s, 1:40 + 10 * s] = rng.integers(0, 90, 39 + 10 * s)
        t[s, bins - 1] = 3 + s
    return t


def _store_flags(store):
    return {"rows": 0, "bins": abi.FLAG_BIN_STORE, "refdraws": abi.FLAG_REFERENCE_DRAWS}[store]


def _spec(store, kmax, with_target, m, flags=abi.FLAG_SNAPSHOT_ROWS | abi.FLAG_EVENT_HASH, **kw):
    """The shape of the ABC-statistics tests: the 300-copy cell reaches the overflow bin; extinct replicates, and the
    snapshot at max_cells (the stop check comes before the snapshot rule), are not taken; the snapshot
    at 4 cells is the initial state."""
    base = dict(seed=4, process=abi.BIRTH_DEATH, rates=((1.0, 1.4, 0.3, 0.3), (1.0, 2.0, 0.5, 0.2)), reps_per_set=300,
                n_replicates=600, max_cells=2000, hist_bins=BINS, init={1: 3, 300: 1}, snapshots=SNAPS,
                flags=abi.FLAG_REP_STATS | flags | _store_flags(store), bin_kmax=kmax, snapshot_stats=True,
                snapshot_targets=_targets(BINS, len(SNAPS)) if with_target else None, snapshot_subsample_cells=m)
    base.update(kw)
    return abi.RunSpec(**base)
