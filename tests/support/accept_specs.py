"""The runs of tests/test_gpu_accept.py and tests/test_gpu_select.py, which cross-check each other on the same shapes:
3,000 or 192 replicates grown to 300 cells, and a source's records from the context's ordinary downloads."""
import numpy as np

from ecdna_evo_amd import abi
from support.gpu import _flags

BINS = 65
C3 = (1.0, 1.5, 0.3, 0.3)
BD_RATES = (C3, (1.0, 1.2, 0.2, 0.4))
DYING = ((1.0, 1.0, 1.1, 1.1), (0.8, 1.0, 1.0, 1.3))  # tests/test_gpu_passages.py: d > b, extinctions


def _targets(rows, bins=BINS):
    rng = np.random.default_rng(23)
    t = rng.integers(0, 60, (rows, bins)).astype(np.uint64)
    t[:, 0] += 100
    t[:, 40:] = 0
    t[:, bins - 1] = 2
    return t


def _final_spec(store="rows", **kw):
    """Birth-death replicates scored at the end of the run and on a 40-cell sample; three sets, the middle one with an
    empty initial distribution (all its replicates end with ECDNA_REP_ERR_EMPTY)."""
    d = dict(seed=7, process=abi.BIRTH_DEATH, segregation=abi.SEG_BINOMIAL, rates=BD_RATES + (C3,), reps_per_set=1000,
             n_replicates=3000, max_cells=300, hist_bins=BINS, flags=_flags(store), bin_kmax=32,
             init_per_set=[{1: 1}, {}, {0: 1, 2: 2}], stats_target=_targets(1)[0], subsample_cells=40)
    d.update(kw)
    return abi.RunSpec(**d)


def _small_spec(n, store="rows", **kw):
    """One or two sets of error-free and extinct replicates, no per-set initial distributions."""
    d = dict(seed=9, process=abi.BIRTH_DEATH, segregation=abi.SEG_BINOMIAL, rates=BD_RATES, reps_per_set=max(1, (n + 1) // 2),
             n_replicates=n, max_cells=300, hist_bins=BINS, flags=_flags(store), bin_kmax=32, init={0: 1, 1: 2},
             stats_target=_targets(1)[0], subsample_cells=40)
    d.update(kw)
    return abi.RunSpec(**d)


def _snapshot_spec(**kw):
    d = dict(seed=4, process=abi.BIRTH_DEATH, rates=((1.0, 1.4, 0.3, 0.3), (1.0, 2.0, 0.5, 0.2)), reps_per_set=96,
             n_replicates=192, max_cells=300, hist_bins=BINS, init={1: 3, 70: 1}, snapshots=(8, 60, 200),
             flags=_flags("bins"), bin_kmax=32, snapshot_stats=True, snapshot_targets=_targets(3),
             snapshot_subsample_cells=40)
    d.update(kw)
    return abi.RunSpec(**d)


def _passage_spec(**kw):
    d = dict(seed=11, process=abi.BIRTH_DEATH, segregation=abi.SEG_BINOMIAL, rates=DYING, reps_per_set=96,
             n_replicates=192, max_cells=300, hist_bins=BINS, cell_cap=4096, flags=_flags("rows"), init={0: 10, 1: 10},
             n_passages=3, passage_cells=40, passage_targets=_targets(3))
    d.update(kw)
    return abi.RunSpec(**d)


def _source(res, source):
    """(records [n][T], summaries [n] or [n][T]) of a source, from the context's ordinary downloads."""
    if source == abi.ACCEPT_FINAL:
        return res.stats[:, None], res.summaries
    if source == abi.ACCEPT_SAMPLE:
        return res.sample_stats[:, None], res.summaries
    if source == abi.ACCEPT_SNAPSHOTS:
        return res.snapshot_stats, res.summaries
    if source == abi.ACCEPT_SNAPSHOT_SAMPLES:
        return res.snapshot_sample_stats, res.summaries
    ps = res.passages
    stats = ps.stats if source == abi.ACCEPT_PASSAGES else ps.sample_stats
    return np.ascontiguousarray(stats.T), np.ascontiguousarray(ps.summaries.T)
