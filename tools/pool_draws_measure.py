"""What pooling the accepted thinnings costs in one pass (ecdna_ssa_ctx_pool_draws, thinned pooling mapping v1) on one
MI355X (docs/PERF_LOG.md). Not a pass/fail gate: it prints what it finds.

The two shapes of tools/accept_draws_measure.py, each launched once:
  keep      bench.py's c3 spec (2^20 replicates to 1e4 cells) with ECDNA_FLAG_REP_STATS and keep_cells = 200; one target
            on m1 = 80 cells, 64 draws.
  snapshots the same rates, 2^17 replicates, T = 4 snapshots with keep_timepoint_cells = 200, each timepoint on 80 cells,
            joint acceptance.
Per shape, at a row of about 1 % acceptance (the KS distance at select's 1 % order statistic of the draw-0 records,
the other statistics off) and at the all-+inf row: the time of ecdna_ssa_ctx_pool_draws with both outputs, with
out_kept alone and with out_thinned alone; beside them ecdna_ssa_ctx_accept_draws at Q = 1 with the same row, on the
same build; and, for out_kept, the loop it replaces: 64 x (sized rescore + accept + pool_accepted). The call is
synchronous, so its time is taken with HIP events around the call on the launch stream, as the enqueued work of the
others is; medians of REPEATS after one warm-up. out_kept is checked against the loop's sum before anything is reported.

Usage: python tools/pool_draws_measure.py [--replicates N] [--out FILE]   (N: the keep shape's; default 2^20)"""
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

import bench  # noqa: E402
from ecdna_evo_amd import abi, engine  # noqa: E402

REPEATS = 5
KEEP, M1, DRAWS = 200, 80, 64
SNAPSHOTS = (1000, 2000, 4000, 8000)
INF = [np.inf] * 4


def target(bins):
    """A patient-like target: most cells with few copies, a thin tail, a few in the overflow bin."""
    k = np.arange(bins, dtype=np.float64)
    t = np.floor(4000.0 * np.exp(-k / 10.0)).astype(np.uint64)
    t[0] = 3000
    t[bins - 1] = 5
    return t


def device_ms(fn):
    import torch  # the engine's default stream is torch's: HIP events around the call

    out = []
    for _ in range(REPEATS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(statistics.median(out[1:]), 3), [round(x, 3) for x in out[1:]]


def pool_only(ctx, block, q, want_thinned, want_kept):
    """ecdna_ssa_ctx_pool_draws with one output NULL (Context.pool_draws always asks for both)."""
    a, alive, thinned, kept = block
    L = engine.lib()
    rc = L.ecdna_ssa_ctx_pool_draws(ctx.h, a, q, thinned.ctypes.data if want_thinned else None,
                                    kept.ctypes.data if want_kept else None)
    assert rc == abi.OK, L.ecdna_ssa_last_error_message().decode()


def measure(name, ctx, n, t, store, rescore, source, pool_accepted):
    import ctypes as C

    p = ctx.params
    slices = t.shape[0] if store == "timepoints" else 1
    # (the KS distance alone at its 1 % order statistic: the other three switched off, or the joint row passes far less)
    one_percent = [float(ctx.select(source, fractions=(0.01,)).values[0, 0])] + INF[1:]
    rows = []
    for label, row in (("about 1 %", one_percent), ("all +inf", INF)):
        thr = np.asarray([row], dtype=np.float64)
        a, alive = ctx._accept_draws_block(t, M1, thr, DRAWS, 0, None, store)
        block = (C.byref(a), alive, np.zeros((t.shape[0], p.n_param_sets, p.hist_bins), dtype=np.uint64),
                 np.zeros((slices, p.n_param_sets, p.hist_bins), dtype=np.uint64))

        def loop():
            total = np.zeros((slices, p.n_param_sets, p.hist_bins), dtype=np.uint64)
            for d in range(DRAWS):
                rescore(d)
                ctx.accept_enqueue(source, thr)
                total += pool_accepted(0).reshape(total.shape)
            return total

        got = ctx.pool_draws(t, M1, thr, 0, DRAWS, 0, None, store)
        assert np.array_equal(got.kept, loop()), f"{name}, {label}: out_kept is not the loop's sum"
        passes = ctx.accept_draws(t, M1, thr, DRAWS, store=store).passes[:, 0]
        both_ms, both_all = device_ms(lambda: pool_only(ctx, block, 0, True, True))
        kept_ms, kept_all = device_ms(lambda: pool_only(ctx, block, 0, False, True))
        thin_ms, thin_all = device_ms(lambda: pool_only(ctx, block, 0, True, False))
        acc_ms, acc_all = device_ms(lambda: ctx.accept_draws_enqueue(t, M1, thr, DRAWS, 0, None, store))
        loop_ms, loop_all = device_ms(loop)
        rows.append({
            "shape": name, "row": label, "replicates": n, "draws": DRAWS, "m1": M1, "keep_cells": KEEP,
            "n_param_sets": int(p.n_param_sets), "hist_bins": int(p.hist_bins),
            "passes_mean": round(float(passes.mean()), 3), "passing_share": round(float((passes > 0).mean()), 4),
            "pool_draws_ms": both_ms, "pool_draws_all_ms": both_all,
            "pool_draws_kept_only_ms": kept_ms, "pool_draws_kept_only_all_ms": kept_all,
            "pool_draws_thinned_only_ms": thin_ms, "pool_draws_thinned_only_all_ms": thin_all,
            "accept_draws_q1_ms": acc_ms, "accept_draws_q1_all_ms": acc_all,
            "loop_kept_ms": loop_ms, "loop_kept_all_ms": loop_all,
            "thinned_cells_pooled": int(got.thinned.sum()), "kept_cells_pooled": int(got.kept.sum()),
        })
    return rows


def keep_shape(n):
    spec = bench.workload_spec(0, n, n, workload="c3")
    spec.flags |= abi.FLAG_REP_STATS
    spec.keep_cells = KEEP
    t = np.ascontiguousarray(target(spec.hist_bins)[None, :])
    with engine.Context(spec) as ctx:
        ctx.launch()
        ctx.sync()
        ctx.rescore(t, M1, 0)
        return measure("keep", ctx, n, t, "keep", lambda d: ctx.rescore_enqueue(t, M1, (d,)), abi.ACCEPT_RESCORED,
                       ctx.pool_accepted)


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
        return measure("snapshots T=4", ctx, n, t, "timepoints", lambda d: ctx.rescore_timepoints_enqueue(t, M1, d),
                       abi.ACCEPT_RESCORED_TIMEPOINTS, ctx.pool_accepted_timepoints)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    lines = []
    for out in keep_shape(args.replicates) + snapshot_shape(max(1024, args.replicates >> 3)):
        out.update(tool="pool_draws_measure", repeats=REPEATS, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
