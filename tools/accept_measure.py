"""What the acceptance pass (ecdna_ssa_ctx_accept) saves a single GPU's host, measured on the C4 sweep's shape
(docs/PERF_LOG.md). Not a pass/fail gate: it prints what it finds.

bench.py's c4 spec with ECDNA_FLAG_REP_STATS and a target is launched once. On that context, wall-clock medians of
REPEATS rounds that alternate the two paths, after one warm-up round:
  (a) ecdna_ssa_ctx_accept + ecdna_ssa_ctx_download_accept with Q = 8 threshold rows and list_capacity = 1 % of n
      (counts, mask, ids and records all downloaded);
  (b) the path before the pass: ecdna_ssa_ctx_download_stats (64 B per replicate) + the numpy restatement of the same
      rule (tests/accept_law.py). The summaries (the error words) are downloaded once outside the timing, which
      favours (b).
and the pass's device time (HIP events on the launch stream around the enqueue). (a)'s results are checked against
(b)'s before anything is reported.

Usage: python tools/accept_measure.py [--replicates N] [--out FILE]   (N a multiple of 1024; default the whole sweep)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "ecdna-evo_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import accept_law as al  # noqa: E402
import bench  # noqa: E402
from ecdna_evo_amd import abi, engine  # noqa: E402

REPEATS = 7
Q = 8


def target_hist(bins):
    """A patient-like target: most cells with few copies, a thin tail, a few in the overflow bin."""
    k = np.arange(bins, dtype=np.float64)
    t = np.floor(4000.0 * np.exp(-k / 12.0)).astype(np.uint64)
    t[0] = 3000
    t[bins - 1] = 5
    return t


def alternating_ms(*fns):
    """Wall-clock times of each function (every one ends in a device synchronise), REPEATS rounds of all of them in turn
    after one warm-up round: per function the median and the times."""
    for fn in fns:
        fn()
    times = [[] for _ in fns]
    for _ in range(REPEATS):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), t) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=bench.WORKLOADS["c4"][0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.replicates
    spec = bench.workload_spec(0, n, n, workload="c4")
    spec.flags |= abi.FLAG_REP_STATS
    spec.stats_target = target_hist(spec.hist_bins)
    L = engine.lib()
    with engine.Context(spec) as ctx:
        ctx.launch()
        ssa_ms, hist_ms = ctx.sync()
        p = ctx.params
        sets, rps = int(p.n_param_sets), int(p.reps_per_set)
        summaries = abi.summaries_array(n)
        engine._check(L.ecdna_ssa_ctx_download(ctx.h, summaries.ctypes.data, None, None, None), "download")
        stats = np.zeros(n, dtype=abi.STATS_DTYPE)
        engine._check(L.ecdna_ssa_ctx_download_stats(ctx.h, stats.ctypes.data), "download_stats")
        ok = summaries["error"] == 0
        fracs = np.linspace(0.05, 0.75, Q)
        thr = np.asarray([[np.sort(stats[f][ok])[int(x * (int(ok.sum()) - 1))] for f in al.FIELDS] for x in fracs])
        ids = spec.replicate_ids()
        cap = n // 100
        list_row = Q - 1

        def host_path():
            engine._check(L.ecdna_ssa_ctx_download_stats(ctx.h, stats.ctypes.data), "download_stats")
            return al.accept(stats, summaries, rps, ids, thr, sets, 0, list_row, cap)

        def device_path():
            return ctx.accept(abi.ACCEPT_FINAL, thr, list_threshold=list_row, list_capacity=cap)

        want, got = host_path(), device_path()
        assert np.array_equal(got.mask, want.mask) and np.array_equal(got.counts, want.counts)
        assert got.n_accepted == want.n_accepted and np.array_equal(got.ids, want.ids)
        assert got.stats.tobytes() == np.ascontiguousarray(stats[want.index]).tobytes()

        def download_only():
            engine._check(L.ecdna_ssa_ctx_download_stats(ctx.h, stats.ctypes.data), "download_stats")

        (a_ms, a_all), (b_ms, b_all), (b_download_ms, _) = alternating_ms(device_path, host_path, download_only)

        import torch  # the engine's default stream is torch's: HIP events around the enqueue

        dev = []
        for _ in range(REPEATS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.accept_enqueue(abi.ACCEPT_FINAL, thr, list_threshold=list_row, list_capacity=cap)
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        out = {
            "tool": "accept_measure", "replicates": n, "sets": sets, "Q": Q, "list_capacity": cap,
            "n_accepted": got.n_accepted, "accepted_per_row": got.counts.sum(axis=1).tolist(),
            "accept_plus_download_ms": round(a_ms, 3), "accept_plus_download_all_ms": [round(x, 3) for x in a_all],
            "download_stats_plus_numpy_ms": round(b_ms, 3), "download_stats_plus_numpy_all_ms": [round(x, 3) for x in b_all],
            "download_stats_alone_ms": round(b_download_ms, 3),
            "accept_device_ms": round(statistics.median(dev[1:]), 4), "accept_device_all_ms": [round(x, 4) for x in dev[1:]],
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
