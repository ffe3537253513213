"""What scoring the kept samples on fewer cells costs (ecdna_ssa_ctx_rescore_sized, thinning mapping v1), measured on the
C4 sweep's shape (docs/PERF_LOG.md). Not a pass/fail gate: it prints what it finds.

bench.py's c4 spec with ECDNA_FLAG_REP_STATS and keep_cells = 200 is launched once. On that context, device times (HIP
events on the launch stream around the enqueue; medians of REPEATS after one warm-up) of
  (a) ecdna_ssa_ctx_rescore with P = 8 targets: every target on all kept cells;
  (b) ecdna_ssa_ctx_rescore_sized with the same targets, each on m1 = 100 cells, draw 0: one thinned sample per
      replicate, scored against the eight;
  (c) the same with eight different draws: eight thinned samples per replicate.
The whole-sample targets of a sized call (m1 = keep_cells) are checked to give (a)'s bytes before anything is reported.

Usage: python tools/thin_measure.py [--replicates N] [--out FILE]   (N a multiple of 1024; default 2^20)"""
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
P, KEEP, M1 = 8, 200, 100


def targets(bins):
    """Patient-like targets: most cells with few copies, a thin tail, a few in the overflow bin."""
    k = np.arange(bins, dtype=np.float64)
    t = np.stack([np.floor(4000.0 * np.exp(-k / (8.0 + 2.0 * p))).astype(np.uint64) for p in range(P)])
    t[:, 0] = 3000
    t[:, bins - 1] = 5
    return t


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
    return statistics.median(out[1:]), out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.replicates
    spec = bench.workload_spec(0, n, n, workload="c4")
    spec.flags |= abi.FLAG_REP_STATS
    spec.keep_cells = KEEP
    t = targets(spec.hist_bins)
    with engine.Context(spec) as ctx:
        ctx.launch()
        ssa_ms, hist_ms = ctx.sync()
        headers, _ = ctx.download_kept()
        plain = ctx.rescore(t)
        assert ctx.rescore(t, KEEP).tobytes() == plain.tobytes()
        thinned = ctx.rescore(t, M1)
        nk = headers["nminus"].astype(np.int64) + headers["nplus"]
        assert np.array_equal(thinned[0]["cells"], np.minimum(nk, M1))
        del plain, thinned
        a_ms, a_all = device_ms(lambda: ctx.rescore_enqueue(t))
        b_ms, b_all = device_ms(lambda: ctx.rescore_enqueue(t, M1))
        c_ms, c_all = device_ms(lambda: ctx.rescore_enqueue(t, M1, tuple(range(P))))
        import torch

        out = {
            "tool": "thin_measure", "replicates": n, "P": P, "keep_cells": KEEP, "m1": M1, "bins": int(spec.hist_bins),
            "kept_cells_mean": round(float(nk.mean()), 2), "thinned_share": round(float((nk > M1).mean()), 4),
            "rescore_ms": round(a_ms, 3), "rescore_all_ms": [round(x, 3) for x in a_all],
            "rescore_sized_one_draw_ms": round(b_ms, 3), "rescore_sized_one_draw_all_ms": [round(x, 3) for x in b_all],
            "rescore_sized_eight_draws_ms": round(c_ms, 3),
            "rescore_sized_eight_draws_all_ms": [round(x, 3) for x in c_all],
            "run_ssa_ms": round(ssa_ms, 2), "run_hist_ms": round(hist_ms, 2), "repeats": REPEATS,
            "device": torch.cuda.get_device_name(0),
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
