"""What scoring one sweep against a cohort of P targets costs next to the sweep itself (ecdna_ssa_cohort_t, ssa_cohort.hip;
docs/PERF_LOG.md). Not a pass/fail gate: it prints what it finds.

One context per P in (0 = no cohort block, 1, 8, 64) on a bin-store birth-death sweep of 2^18 replicates to 1e4 cells,
hist_bins = 128, every target with a sample of 300 cells (one group: the sample is drawn once and scored P times), plus
one context with 64 targets of 64 distinct sample sizes (64 groups: 64 draws per replicate). Each context is launched
LAUNCHES times after one warm-up launch; the line is the median ssa_ms and hist_ms of ecdna_ssa_ctx_sync (HIP events on
the launch stream: the stepper, and the end-of-run passes, the cohort pass among them). The yardsticks are the P = 0 line
of the same run and the launch's own ssa_ms.

Usage: python tools/cohort_cost.py [--replicates N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "ecdna-evo_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from ecdna_evo_amd import abi, engine  # noqa: E402

BINS = 128
SAMPLE = 300
LAUNCHES = 5


def targets(P):
    rng = np.random.default_rng(17)
    t = rng.integers(0, 200, (P, BINS)).astype(np.uint64)
    t[:, 0] += 500
    t[:, 60:BINS - 1] = 0
    t[:, BINS - 1] = 3
    return t


def spec_of(n, P, distinct=False):
    sets = max(1, n // 256)
    rng = np.random.default_rng(5)
    rates = np.stack([np.ones(sets), rng.uniform(1.1, 1.6, sets), rng.uniform(0.1, 0.4, sets),
                      rng.uniform(0.1, 0.4, sets)], axis=1)
    spec = abi.RunSpec(seed=26, process=abi.BIRTH_DEATH, rates=rates, reps_per_set=n // sets, n_replicates=n,
                       max_cells=10_000, hist_bins=BINS, init={1: 1}, bin_kmax=64,
                       flags=abi.FLAG_REP_STATS | abi.FLAG_BIN_STORE, stats_target=targets(1)[0],
                       subsample_cells=SAMPLE)
    if P:
        spec.cohort_targets = targets(P)
        spec.cohort_sample_cells = [SAMPLE + p for p in range(P)] if distinct else [SAMPLE] * P
    return spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for P, distinct in ((0, False), (1, False), (8, False), (64, False), (64, True)):
        with engine.Context(spec_of(args.replicates, P, distinct)) as ctx:
            times = []
            for _ in range(LAUNCHES + 1):
                ctx.launch()
                times.append(ctx.sync())
            ins = ctx.instance()
        ssa = [t[0] for t in times[1:]]
        hist = [t[1] for t in times[1:]]
        lines.append({"tool": "cohort_cost", "replicates": args.replicates, "targets": P,
                      "groups": (P if distinct else min(P, 1)), "sample_cells": SAMPLE, "hist_bins": BINS,
                      "ssa_ms": round(statistics.median(ssa), 3), "hist_ms": round(statistics.median(hist), 3),
                      "ssa_all_ms": [round(x, 3) for x in ssa], "hist_all_ms": [round(x, 3) for x in hist],
                      "n_chunks": ins["n_chunks"], "launches": LAUNCHES})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
