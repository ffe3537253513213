"""The cases of tests/test_gpu_passages.py and their oracle chains, which the timepoint keep suite runs again with the
timepoint keep block."""
import numpy as np

import abc_stats
import passage_law as pl
import subsample_law as sl
from ecdna_evo_amd import abi
from support.gpu import _flags

N, G, MAX_CELLS, BINS, SEED = 192, 3, 300, 65, 11
C3 = (1.0, 1.5, 0.3, 0.3)
BD_RATES = (C3, (1.0, 1.2, 0.2, 0.4))
PB_RATES = ((1.0, 1.0, 0.0, 0.0), (1.0, 1.5, 0.0, 0.0))
DYING = ((1.0, 1.0, 1.1, 1.1), (0.8, 1.0, 1.0, 1.3))  # d > b: extinctions


def _targets(G=G, BINS=BINS):
    rng = np.random.default_rng(17)
    t = rng.integers(0, 60, (G, BINS)).astype(np.uint64)
    t[:, 0] += 100
    t[:, 40:] = 0
    t[:, BINS - 1] = 2
    return t


def _base(store, kmax, process, seg, rates, **kw):
    """The plain run's keywords (no passages, no sample): two parameter sets of 96 replicates (keywords override)."""
    d = dict(seed=SEED, process=process, segregation=seg, rates=rates, reps_per_set=N // 2, n_replicates=N,
             max_cells=MAX_CELLS, hist_bins=BINS, cell_cap=4096, flags=_flags(store), bin_kmax=kmax)
    d.update(kw)
    return d


def _passage_spec(base, m, G=G, **kw):
    targets = _targets(G, base["hist_bins"])
    return abi.RunSpec(**{**base, "n_passages": G, "passage_cells": m, "passage_targets": targets, **kw})


# (id, store, K, process, segregation, rates, m, extra spec keywords)
CASES = [
    ("rows-pb-binomial-picks", "rows", 0, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES, 40, {}),
    ("rows-bd-deterministic-complement", "rows", 0, abi.BIRTH_DEATH, abi.SEG_DETERMINISTIC, BD_RATES, 200, {}),
    ("bins32-bd-binomial-picks", "bins", 32, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES, 40, {}),
    ("bins64-pb-deterministic-complement", "bins", 64, abi.PURE_BIRTH, abi.SEG_DETERMINISTIC, PB_RATES, 200,
     dict(init={3: 2, 70: 1})),
    ("bins64-bd-binomial-complement", "bins", 64, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES, 200, {}),
    ("rows-bd-whole", "rows", 0, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES, 4096, {}),
    ("bins64-pb-whole", "bins", 64, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES, 4096, {}),
    ("rows-extinctions", "rows", 0, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, DYING, 40, dict(init={0: 10, 1: 10})),
    ("bins32-extinctions", "bins", 32, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, DYING, 40, dict(init={0: 10, 1: 10})),
    ("bins32-large-k-founders", "bins", 32, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES, 40, dict(init={40: 3})),
    ("bins32-large-k-cell-cap", "bins", 32, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES, 40,
     dict(init={1: 5, 40: 3}, big_cap=24)),
    # K = 256: the prefix sums of the counters take four 64-lane blocks (u16 counters at cell_cap = 4096); the 300-copy
    # cell lies above K, so both the counters and the large-k row are sampled
    ("bins256-bd-binomial-picks", "bins", 256, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES, 40,
     dict(init={1: 3, 300: 1})),
    ("bins256-bd-deterministic-complement", "bins", 256, abi.BIRTH_DEATH, abi.SEG_DETERMINISTIC, BD_RATES, 200,
     dict(init={1: 3, 300: 1})),
]


_CHAINS = {}


def _sum_sets(per_rep, sets, rps):
    """Per-replicate-set oracle arrays (set i = replicate i) summed into the run's parameter sets."""
    out = np.zeros((sets,) + per_rep.shape[1:], dtype=per_rep.dtype)
    for i in range(per_rep.shape[0]):
        if per_rep.dtype.names:
            for f in per_rep.dtype.names:
                out[f][i // rps] += per_rep[f][i]
        else:
            out[i // rps] += per_rep[i]
    return out


def _chain(oracle_mod, key, base, m, N=N, G=G, MAX_CELLS=MAX_CELLS, BINS=BINS):
    """The oracle chain of a case (computed once, shared, left unchanged): per phase the oracle's summaries, histogram
    [sets][bins], totals [sets] and rows, and the restatements' statistics, sample statistics and sample histogram."""
    if key in _CHAINS:
        return _CHAINS[key]
    assert (base["n_replicates"], base["max_cells"], base["hist_bins"]) == (N, MAX_CELLS, BINS)
    targets = _targets(G, BINS)
    sets, rps = len(base["rates"]), base["reps_per_set"]
    rates_of = [base["rates"][i // rps] for i in range(N)]
    phases = []
    o = oracle_mod.run(abi.RunSpec(**base), want_rows=True)
    hist, totals = o.hist.copy(), o.totals.copy()
    for g in range(G):
        sg = pl.seed_g(SEED, g)
        stats, sstats = [], []
        shist = np.zeros((sets, BINS), dtype=np.uint64)
        inits = []
        for i in range(N):
            nm, row = int(o.summaries[i]["nminus"]), o.row(i)
            stats.append(abc_stats.rep_stats(nm, row, BINS, targets[g]))
            sstats.append(sl.sample_stats(nm, row, m, sg, i, BINS, targets[g]))
            shist[i // rps] += sl.sample_hist(nm, row, m, sg, i, BINS)
            inits.append(pl.founders_hist(nm, row, m, SEED, g, i))
        phases.append(dict(summaries=o.summaries.copy(), hist=hist, totals=totals, rows=[o.row(i).copy() for i in range(N)],
                           stats=stats, sample_stats=sstats, sample_hist=shist, founders=inits))
        if g + 1 < G:
            nxt = {**base, "seed": pl.seed_g(SEED, g + 1), "rates": rates_of, "reps_per_set": 1, "init_per_set": inits}
            nxt.pop("init", None)
            o = oracle_mod.run(abi.RunSpec(**nxt), want_rows=True)
            hist, totals = _sum_sets(o.hist, sets, rps), _sum_sets(o.totals, sets, rps)
    _CHAINS[key] = phases
    return phases
