"""What counting acceptance over 64 thinning draws costs in one pass (ecdna_ssa_ctx_accept_draws, thinned acceptance
mapping v1) against the loop it replaces, on one MI355X (docs/PERF_LOG.md). Not a pass/fail gate: it prints
what it finds.

Two shapes, each launched once:
  keep      bench.py's c3 spec (2^20 replicates to 1e4 cells) with ECDNA_FLAG_REP_STATS and keep_cells = 200; one target
            on m1 = 80 cells, 64 draws, Q = 8 rows. The loop: one ecdna_ssa_ctx_rescore_sized with the target in all 64
            slots and sample_draws = 0 .. 63, then 64 ecdna_ssa_ctx_accept (timepoint_mask = 1 << p), each with its mask
            download, summed on the host.
  snapshots the same rates, 2^17 replicates, T = 4 snapshots with keep_timepoint_cells = 200, each timepoint on 80 cells,
            joint acceptance. The loop: 64 times ecdna_ssa_ctx_rescore_timepoints_sized, accept and the mask download.
Per shape: wall-clock of the whole exchange (enqueue to the counts on the host) and device time of the enqueued work
alone (HIP events on the launch stream), medians of REPEATS after one warm-up. The fused counts are checked against the
loop's before anything is reported. The records' bytes are the calls' own arithmetic.

Usage: python tools/accept_draws_measure.py [--replicates N] [--out FILE]   (N: the keep shape's; default 2^20)"""
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
from ecdna_evo_amd import abi, engine  # noqa: E402

REPEATS = 5
KEEP, M1, DRAWS, Q = 200, 80, 64, 8
FRACTIONS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)
SNAPSHOTS = (1000, 2000, 4000, 8000)


def target(bins):
    """A patient-like target: most cells with few copies, a thin tail, a few in the overflow bin."""
    k = np.arange(bins, dtype=np.float64)
    t = np.floor(4000.0 * np.exp(-k / 10.0)).astype(np.uint64)
    t[0] = 3000
    t[bins - 1] = 5
    return t


def timed(fn):
    """(median wall ms, all) of fn() — which ends with its results on the host — after one warm-up."""
    out = []
    for _ in range(REPEATS + 1):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out[1:]), [round(x, 3) for x in out[1:]]


def device_ms(enqueue):
    import torch  # the engine's default stream is torch's: HIP events around the enqueue

    out = []
    for _ in range(REPEATS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enqueue()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out[1:]), [round(x, 3) for x in out[1:]]


def bits(mask):
    return ((mask[:, None] >> np.arange(Q, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.uint8)


def measure(name, ctx, fused, fused_enqueue, loop, loop_enqueue, loop_bytes, n):
    want = loop()
    got = fused()
    assert np.array_equal(got.passes, want), f"{name}: the fused counts are not the loop's"
    f_ms, f_all = timed(fused)
    l_ms, l_all = timed(loop)
    fd_ms, fd_all = device_ms(fused_enqueue)
    ld_ms, ld_all = device_ms(loop_enqueue)
    p = got.passes
    return {
        "shape": name, "replicates": n, "draws": DRAWS, "Q": Q, "m1": M1, "keep_cells": KEEP,
        "fused_wall_ms": round(f_ms, 3), "fused_wall_all_ms": f_all, "loop_wall_ms": round(l_ms, 3),
        "loop_wall_all_ms": l_all, "fused_device_ms": round(fd_ms, 3), "fused_device_all_ms": fd_all,
        "loop_device_ms": round(ld_ms, 3), "loop_device_all_ms": ld_all,
        "fused_result_bytes": int(n * Q + Q * ctx.params.n_param_sets * 8), "loop_record_bytes": int(loop_bytes),
        "passes_mean_per_row": [round(float(x), 3) for x in p.mean(axis=0)],
        "partial_share_per_row": [round(float(x), 4) for x in ((p > 0) & (p < DRAWS)).mean(axis=0)],
    }


def keep_shape(n):
    spec = bench.workload_spec(0, n, n, workload="c3")
    spec.flags |= abi.FLAG_REP_STATS
    spec.keep_cells = KEEP
    t = target(spec.hist_bins)[None, :]
    t64 = np.ascontiguousarray(np.repeat(t, DRAWS, axis=0))
    with engine.Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        ctx.rescore(t, M1, 0)
        thr = np.ascontiguousarray(ctx.select(abi.ACCEPT_RESCORED, fractions=FRACTIONS).values.T)

        def loop_enqueue():
            ctx.rescore_enqueue(t64, M1, tuple(range(DRAWS)))
            for p in range(DRAWS):
                ctx.accept_enqueue(abi.ACCEPT_RESCORED, thr, [p])

        def loop():
            ctx.rescore_enqueue(t64, M1, tuple(range(DRAWS)))
            total = np.zeros((n, Q), dtype=np.uint8)
            for p in range(DRAWS):
                total += bits(ctx.accept(abi.ACCEPT_RESCORED, thr, [p]).mask)
            return total

        return measure("keep", ctx, lambda: ctx.accept_draws(t, M1, thr, DRAWS),
                       lambda: ctx.accept_draws_enqueue(t, M1, thr, DRAWS), loop, loop_enqueue,
                       DRAWS * n * abi.STATS_DTYPE.itemsize, n)


def snapshot_shape(n):
    spec = bench.workload_spec(0, n, n, workload="c3")
    spec.flags |= abi.FLAG_REP_STATS
    spec.snapshots = SNAPSHOTS
    spec.snapshot_stats = True
    spec.keep_timepoint_cells = KEEP
    T = len(SNAPSHOTS)
    t = np.ascontiguousarray(np.repeat(target(spec.hist_bins)[None, :], T, axis=0))
    with engine.Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        ctx.rescore_timepoints(t, M1, 0)
        thr = np.ascontiguousarray(ctx.select(abi.ACCEPT_RESCORED_TIMEPOINTS, fractions=FRACTIONS).values.T)

        def loop_enqueue():
            for d in range(DRAWS):
                ctx.rescore_timepoints_enqueue(t, M1, d)
                ctx.accept_enqueue(abi.ACCEPT_RESCORED_TIMEPOINTS, thr)

        def loop():
            total = np.zeros((n, Q), dtype=np.uint8)
            for d in range(DRAWS):
                ctx.rescore_timepoints_enqueue(t, M1, d)
                total += bits(ctx.accept(abi.ACCEPT_RESCORED_TIMEPOINTS, thr).mask)
            return total

        return measure("snapshots T=4", ctx, lambda: ctx.accept_draws(t, M1, thr, DRAWS, store="timepoints"),
                       lambda: ctx.accept_draws_enqueue(t, M1, thr, DRAWS, store="timepoints"), loop, loop_enqueue,
                       T * n * abi.STATS_DTYPE.itemsize, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    lines = []
    for out in (keep_shape(args.replicates), snapshot_shape(max(1024, args.replicates >> 3))):
        out.update(tool="accept_draws_measure", repeats=REPEATS, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
