"""What choosing ABC thresholds on the GPU (ecdna_ssa_ctx_select) costs next to the two paths a caller had before,
measured on the C4 sweep's shape (docs/PERF_LOG.md). Not a pass/fail gate: it prints what it finds.

bench.py's c4 spec with ECDNA_FLAG_REP_STATS, a target and a 40-cell end-of-run sample (so that the context holds a
second source) is launched once. On that context, for K = 8 ranks (fractions 0.1 %, 0.5 %, 1 %, 2 %, 5 %, 10 %, 25 %,
50 % of the error-free replicates) of the final source, wall-clock medians of REPEATS rounds that alternate the paths,
after one warm-up round:
  (a) Context.select. Each timed call follows a one-rank select of the other source, so it makes its keys anew, as the
      first call after a launch does; (a_warm) is the same call repeated, with the keys in place.
  (b) the path it replaces: ecdna_ssa_ctx_download_stats (64 B per replicate) + np.partition for the same ranks on the
      four fields. The summaries (the error words) are downloaded once outside the timing, which favours (b).
  (c) a host bisection built from ecdna_ssa_ctx_accept: per round one call with 32 threshold rows, 8 per statistic, each
      with that statistic's probe as its one finite threshold, and only the counts downloaded; it bisects the f64 bit
      patterns (monotone for the non-negative distances) until every probe is the exact order statistic.
and the device timeline of single passes (HIP events on the launch stream around one ecdna_ssa_ctx_select_digits call:
the histogram's memset, the kernel, the histogram's copy to the host), with the keys in place and with the keys made
anew. (a)'s values are checked against (b)'s and (c)'s, bit for bit, before anything is reported.

Usage: python tools/select_measure.py [--replicates N] [--out FILE]   (N a multiple of 1024; default the whole sweep)"""
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

import bench  # noqa: E402
from ecdna_evo_amd import abi, engine  # noqa: E402

from accept_measure import REPEATS, alternating_ms, target_hist  # noqa: E402

FRACTIONS = (0.001, 0.005, 0.01, 0.02, 0.05, 0.10, 0.25, 0.50)
K = len(FRACTIONS)
INF = np.inf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=bench.WORKLOADS["c4"][0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.replicates
    spec = bench.workload_spec(0, n, n, workload="c4")
    spec.flags |= abi.FLAG_REP_STATS
    spec.stats_target = target_hist(spec.hist_bins)
    spec.subsample_cells = 40
    L = engine.lib()
    with engine.Context(spec) as ctx:
        ctx.launch()
        ssa_ms, hist_ms = ctx.sync()
        sets = int(ctx.params.n_param_sets)
        summaries = abi.summaries_array(n)
        engine._check(L.ecdna_ssa_ctx_download(ctx.h, summaries.ctypes.data, None, None, None), "download")
        ok = summaries["error"] == 0
        M = int(ok.sum())
        ranks = [max(1, int(np.ceil(f * float(M)))) for f in FRACTIONS]
        stats = np.zeros(n, dtype=abi.STATS_DTYPE)

        def other_source():
            ctx.select(abi.ACCEPT_SAMPLE, ranks=[1])

        def device_cold():
            other_source()
            t0 = time.perf_counter()
            r = ctx.select(abi.ACCEPT_FINAL, ranks=ranks)
            return r, (time.perf_counter() - t0) * 1e3

        def device_warm():
            return ctx.select(abi.ACCEPT_FINAL, ranks=ranks)

        def host_path():
            engine._check(L.ecdna_ssa_ctx_download_stats(ctx.h, stats.ctypes.data), "download_stats")
            idx = np.asarray(ranks) - 1
            return np.asarray([np.partition(stats[f][ok], idx)[idx] for f in abi.SELECT_FIELDS])

        def download_only():
            engine._check(L.ecdna_ssa_ctx_download_stats(ctx.h, stats.ctypes.data), "download_stats")

        rounds = [0]

        def bisection():
            """The smallest bit pattern whose threshold accepts >= rank replicates, per statistic and rank."""
            lo = np.zeros((4, K), dtype=np.uint64)
            hi = np.full((4, K), np.asarray([np.finfo(np.float64).max]).view(np.uint64)[0], dtype=np.uint64)
            counts = np.zeros((4 * K, sets), dtype=np.uint64)
            rounds[0] = 0
            while (lo < hi).any():
                mid = lo + (hi - lo) // np.uint64(2)
                thr = np.full((4 * K, 4), INF)
                for x in range(4):
                    thr[x * K:(x + 1) * K, x] = mid[x].view(np.float64)
                ctx.accept_enqueue(abi.ACCEPT_FINAL, thr)
                engine._check(L.ecdna_ssa_ctx_download_accept(ctx.h, counts.ctypes.data, None, None, None, None),
                              "download_accept")
                enough = counts.sum(axis=1).reshape(4, K) >= np.asarray(ranks, dtype=np.uint64)[None, :]
                hi = np.where(enough, mid, hi)
                lo = np.where(enough, lo, mid + np.uint64(1))
                rounds[0] += 1
            return lo.view(np.float64)

        got, _ = device_cold()
        assert got.population == M and got.ranks.tolist() == ranks
        assert got.values.tobytes() == np.ascontiguousarray(host_path()).tobytes()
        assert got.values.tobytes() == np.ascontiguousarray(bisection()).tobytes()
        by_fraction = ctx.select(abi.ACCEPT_FINAL, fractions=FRACTIONS)
        assert by_fraction.ranks.tolist() == ranks and by_fraction.values.tobytes() == got.values.tobytes()

        cold = [device_cold()[1] for _ in range(REPEATS + 1)][1:]
        (w_ms, w_all), (b_ms, b_all), (b_download_ms, _), (c_ms, c_all) = alternating_ms(
            device_warm, host_path, download_only, bisection)

        import torch  # the engine's default stream is torch's: HIP events around a call

        def pass_ms(pass_, prefixes, rebuild):
            out = []
            for _ in range(REPEATS + 1):
                if rebuild:
                    other_source()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.select_digits(abi.ACCEPT_FINAL, pass_, prefixes)
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return out[1:]

        sign = np.uint64(1 << 63)
        keys = np.ascontiguousarray(got.values).view(np.uint64) ^ sign  # (the selected values are non-negative)
        first = pass_ms(0, keys, False)
        last = pass_ms(7, keys, False)
        first_rebuilt = pass_ms(0, keys, True)
        out = {
            "tool": "select_measure", "replicates": n, "sets": sets, "K": K, "population": M, "ranks": ranks,
            "values_ks": got.values[0].tolist(), "counts_le_ks": got.counts_le[0].tolist(),
            "select_ms": round(statistics.median(cold), 3), "select_all_ms": [round(x, 3) for x in cold],
            "select_keys_in_place_ms": round(w_ms, 3), "select_keys_in_place_all_ms": [round(x, 3) for x in w_all],
            "download_stats_plus_partition_ms": round(b_ms, 3),
            "download_stats_plus_partition_all_ms": [round(x, 3) for x in b_all],
            "download_stats_alone_ms": round(b_download_ms, 3),
            "accept_bisection_ms": round(c_ms, 3), "accept_bisection_all_ms": [round(x, 3) for x in c_all],
            "accept_bisection_rounds": rounds[0],
            "pass0_device_ms": round(statistics.median(first), 4), "pass0_device_all_ms": [round(x, 4) for x in first],
            "pass7_device_ms": round(statistics.median(last), 4), "pass7_device_all_ms": [round(x, 4) for x in last],
            "pass0_with_keys_device_ms": round(statistics.median(first_rebuilt), 4),
            "pass0_with_keys_device_all_ms": [round(x, 4) for x in first_rebuilt],
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
