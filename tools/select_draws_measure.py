"""What finding ABC thresholds over 64 thinning draws costs in one call (ecdna_ssa_ctx_select_draws, thinned select
mapping v1) against the loop it replaces, on one MI355X (docs/PERF_LOG.md). Not a pass/fail gate: it prints
what it finds.

Two shapes, those of tools/accept_draws_measure.py, each launched once:
  keep      bench.py's c3 spec (2^20 replicates to 1e4 cells) with ECDNA_FLAG_REP_STATS and keep_cells = 200; one target
            on m1 = 80 cells, 64 draws, K = 8 fractions.
  snapshots the same rates, 2^17 replicates, T = 4 snapshots with keep_timepoint_cells = 200, each timepoint on 80 cells,
            the key the maximum over the four.
Per shape, medians of REPEATS after one warm-up, HIP events on the launch stream around each (synchronous) call and the
wall clock beside them:
  select_draws   the whole call: the keys once, eight digit passes, the walk
  pass0          ecdna_ssa_ctx_select_draws_digits pass 0: the keys and one digit pass (one prefix)
  passes1_7      its passes 1 .. 7 on the walk's prefixes: seven digit passes over the cached keys
  keys (derived) pass0 less one seventh of passes1_7; digits8 (derived) eight sevenths of passes1_7
  accept_inf     ecdna_ssa_ctx_accept_draws with one all-+inf row, to its results on the host: the pass the keys pass
                 was expected to cost about as much as
  loop           64 x (the sized rescore at draw d + 8 x ecdna_ssa_ctx_select_digits on the rescored records), existing
                 calls only. A loop cannot know pass p's prefixes before every draw's pass p - 1 is summed, so a real one
                 rescored eight times over or held every draw's records; this one is handed the walk's prefixes and is the
                 cheapest form of it.
Before anything is reported the loop's digit arrays, summed over the draws, are checked against the call's own, pass by
pass (contract S1 at this size), and the walk over them against select_draws' result.

Usage: python tools/select_draws_measure.py [--replicates N] [--out FILE]   (N: the keep shape's; default 2^20; FILE is
appended to)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "ecdna-evo_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from ecdna_evo_amd import abi, engine, shard  # noqa: E402

REPEATS = 5
KEEP, M1, DRAWS = 200, 80, 64
FRACTIONS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)
SNAPSHOTS = (1000, 2000, 4000, 8000)
PASSES = shard.SelectWalk.PASSES


def target(bins):
    """A patient-like target: most cells with few copies, a thin tail, a few in the overflow bin."""
    k = np.arange(bins, dtype=np.float64)
    t = np.floor(4000.0 * np.exp(-k / 10.0)).astype(np.uint64)
    t[0] = 3000
    t[bins - 1] = 5
    return t


def timed(fn):
    """(median device ms, all, median wall ms, all) of the synchronous fn() after one warm-up: HIP events around it on the
    engine's stream (torch's default), and the wall clock."""
    import torch

    dev, wall = [], []
    for _ in range(REPEATS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return (round(statistics.median(dev[1:]), 3), [round(x, 3) for x in dev[1:]],
            round(statistics.median(wall[1:]), 3), [round(x, 3) for x in wall[1:]])


def measure(name, ctx, n, slots, fused, digits, rescore_at, source, accept_inf):
    K = len(FRACTIONS)
    got = fused()
    walk, prefixes, hists = shard.SelectWalk(K, fractions=FRACTIONS), [], []
    for p in range(PASSES):
        prefixes.append(walk.prefixes)
        hists.append(digits(p, prefixes[p]))
        walk.feed(hists[p])
    res = walk.result()
    assert (res.population, res.values.tobytes(), res.counts_le.tobytes()) == \
        (got.population, got.values.tobytes(), got.counts_le.tobytes()), f"{name}: the walk is not select_draws'"

    def loop(check=False):
        total = [np.zeros_like(h) for h in hists]
        for d in range(DRAWS):
            rescore_at(d)
            for p in range(PASSES):
                total[p] += ctx.select_digits(source, p, prefixes[p])
        if check:
            for p in range(PASSES):
                assert np.array_equal(total[p], hists[p]), f"{name}: pass {p} of the loop is not the call's (S1)"

    loop(check=True)
    out = {"shape": name, "replicates": n, "draws": DRAWS, "K": K, "m1": M1, "keep_cells": KEEP, "slots": slots,
           "population": int(got.population), "keys_bytes": int(32 * n * DRAWS),
           "loop_record_bytes": int(slots * n * abi.STATS_DTYPE.itemsize),
           "values_ks": [float(v) for v in got.values[0]]}
    for key, fn in (("select_draws", fused), ("pass0", lambda: digits(0, prefixes[0])),
                    ("passes1_7", lambda: [digits(p, prefixes[p]) for p in range(1, PASSES)]),
                    ("accept_inf", accept_inf), ("loop", loop)):
        if key == "passes1_7":
            digits(0, prefixes[0])  # (the keys of this block, whatever ran before)
        d, d_all, w, w_all = timed(fn)
        out.update({f"{key}_device_ms": d, f"{key}_device_all_ms": d_all, f"{key}_wall_ms": w, f"{key}_wall_all_ms": w_all})
    out["keys_derived_device_ms"] = round(out["pass0_device_ms"] - out["passes1_7_device_ms"] / 7.0, 3)
    out["digits8_derived_device_ms"] = round(out["passes1_7_device_ms"] * 8.0 / 7.0, 3)
    return out


def keep_shape(n):
    spec = bench.workload_spec(0, n, n, workload="c3")
    spec.flags |= abi.FLAG_REP_STATS
    spec.keep_cells = KEEP
    t = target(spec.hist_bins)[None, :]
    inf = np.full((1, 4), np.inf)
    with engine.Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        return measure("keep", ctx, n, 1, lambda: ctx.select_draws(t, M1, DRAWS, fractions=FRACTIONS),
                       lambda p, pre: ctx.select_draws_digits(t, M1, p, pre, DRAWS),
                       lambda d: ctx.rescore_enqueue(t, M1, d), abi.ACCEPT_RESCORED,
                       lambda: ctx.accept_draws(t, M1, inf, DRAWS))


def snapshot_shape(n):
    spec = bench.workload_spec(0, n, n, workload="c3")
    spec.flags |= abi.FLAG_REP_STATS
    spec.snapshots = SNAPSHOTS
    spec.snapshot_stats = True
    spec.keep_timepoint_cells = KEEP
    T = len(SNAPSHOTS)
    t = np.ascontiguousarray(np.repeat(target(spec.hist_bins)[None, :], T, axis=0))
    inf = np.full((1, 4), np.inf)
    with engine.Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        return measure("snapshots T=4", ctx, n, T,
                       lambda: ctx.select_draws(t, M1, DRAWS, store="timepoints", fractions=FRACTIONS),
                       lambda p, pre: ctx.select_draws_digits(t, M1, p, pre, DRAWS, store="timepoints"),
                       lambda d: ctx.rescore_timepoints_enqueue(t, M1, d), abi.ACCEPT_RESCORED_TIMEPOINTS,
                       lambda: ctx.accept_draws(t, M1, inf, DRAWS, store="timepoints"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    lines = []
    for out in (keep_shape(args.replicates), snapshot_shape(max(1024, args.replicates >> 3))):
        out.update(tool="select_draws_measure", repeats=REPEATS, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
