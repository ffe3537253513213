// ssa_snapstats.hip — the per-replicate ABC statistics at the snapshots (gfx950): the longitudinal half of the
// end-of-run passes (ecdna_ssa_ext_t.snapshot_stats, include/ecdna_ssa.h).
//
// A patient, or a culture experiment, is sampled several times while the tumour grows (abc.md's `timepoint` column),
// and a run is scored against the data of every timepoint. The steppers save a replicate's state at each snapshot as
// an expanded u16 row (snap_rows) with its metadata (snap_meta); this pass, right after ssa_hist and on the same
// stream, reads every (replicate, snapshot) pair of the chunk where it lies and writes its ecdna_rep_stats_t against
// that snapshot's own target, the per-snapshot, per-set sum of the histograms, and — with m > 0 — the same for a
// uniform sample of m cells of the saved state (subsample mapping v1 on the stream of snapshot s,
// ssa_sampledraw.hpp). So the rows of a chunk are scratch: nothing but the statistics has to outlive it.
//
// One wave per (replicate, snapshot) pair, as ssa_hist<true, 0> walks a row. A snapshot that was not taken is an empty
// population (cells 0, ks 1.0 with a target; nothing added to a histogram). Per wave in LDS: the pair's histogram
// (u32 per bin) and the table of the positions drawn so far; per workgroup: the sums of the histograms of one
// (parameter-set segment, snapshot) at a time, flushed with one global atomic per non-zero bin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

constexpr uint32_t kSnapBlock = 256;

// SHIST_LDS: the workgroup's sum of the samples' histograms lies in LDS (hbs); else the waves add their samples' bins
// to global memory (the largest histogram beside the largest table does not leave room for it).
template <bool SHIST_LDS>
__global__ void __launch_bounds__(kSnapBlock) ssa_snapstats(const SnapStatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const ChunkIds& ids = a.ids;
    unsigned long long* hb = lds;              // [bins] the saved states' histograms
    unsigned long long* hbs = lds + ids.bins;  // [bins] the samples' (SHIST_LDS and m > 0)
    const bool sampling = a.m != 0u;
    const uint32_t n_hb = (sampling && SHIST_LDS) ? 2u * ids.bins : ids.bins;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t wave_words = ids.bins + a.table_slots;
    uint32_t* wh = reinterpret_cast<uint32_t*>(lds + n_hb) + (size_t)wave * wave_words;  // [bins]
    uint32_t* tab = wh + ids.bins;                                                       // [table_slots]
    const uint32_t r_begin = blockIdx.x * ids.reps_per_block;
    if (r_begin >= ids.n) return;
    const uint32_t r_end = min(ids.n, r_begin + ids.reps_per_block);
    const uint32_t last = ids.bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    uint32_t r = r_begin;
    while (r < r_end) {
        const auto [set, seg_end] = set_segment(ids.rid0, ids.rid_stride, ids.reps_per_set, r, r_end);
        for (uint32_t s = 0; s < a.n_snap; ++s) {
            const uint64_t out_bins = ((uint64_t)s * a.n_sets + set) * ids.bins;  // hist[s][set][0]
            const StatsTarget target = a.target_cdf ? StatsTarget{a.target_cdf + (uint64_t)s * ids.bins,
                                                                  a.target_scalars[3u * s], a.target_scalars[3u * s + 1u],
                                                                  a.target_scalars[3u * s + 2u], 1u}
                                                    : StatsTarget{};
            for (uint32_t b = tid; b < n_hb; b += blockDim.x) lds[b] = 0ull;
            __syncthreads();
            unsigned long long* sample_sum =
                SHIST_LDS ? hbs : (sampling ? reinterpret_cast<unsigned long long*>(a.sample_hist + out_bins) : nullptr);
            for (uint32_t q = r + wave; q < seg_end; q += nw) {
                const uint64_t pair = (uint64_t)q * a.n_snap + s;
                const ecdna_snapshot_t* meta = a.snap_meta + pair;
                const bool taken = meta->taken != 0u;
                const uint64_t nm = taken ? meta->nminus : 0ull;
                // the cells of the row (never past the row's memory)
                const uint32_t np = taken ? (uint32_t)min(meta->nplus, a.snap_stride) : 0u;
                const uint64_t cells_all = nm + (uint64_t)np;
                const uint16_t* row = a.snap_rows + pair * a.snap_stride;
                for (uint32_t b = lane; b < ids.bins; b += 64u) wh[b] = 0u;
                wave_sync_lds();

                // 1. the saved state's histogram and statistics
                uint64_t ksum = 0;
                wave_row_hist(row, np, last, wh, ksum, lane);
                if (lane == 0 && nm) atomicAdd(&wh[0], (uint32_t)nm);
                wave_sync_lds();
                wave_rep_stats(wh, hb, ids.bins, cells_all, wave_sum(ksum), np, target.has, target.cdf, target.mean,
                               target.entropy, target.freq, lane, a.stats + pair);

                // 2. the sample: the whole population (m >= N; a snapshot not taken has N = 0), the picked positions
                // (m' = m) or what they leave of the histogram above (m' < m)
                if (sampling) {
                    const SamplePlan plan = sample_plan(a.m, cells_all);
                    uint64_t psum = 0;  // sum of k over the picked positions
                    bool bad = plan.bad;
                    if (!plan.whole) {
                        wave_sync_lds();  // the statistics above have read wh
                        if (!plan.comp) {
                            for (uint32_t b = lane; b < ids.bins; b += 64u) wh[b] = 0u;
                            wave_sync_lds();
                        }
                        if (!bad) {
                            const uint64_t rid = ids.rid0 + (uint64_t)q * ids.rid_stride;
                            const SamplePop pop{nm, nullptr, 0u, 0u, row, np};
                            bad = wave_sample_picks<0>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                                       sample_stream_tag(s + 1u), rid, k0, k1, lane, psum);
                        }
                        wave_sync_lds();
                    }
                    wave_sample_stats(plan, bad, a.m, cells_all, np, ksum, psum, wh, sample_sum, ids.bins, target, lane,
                                      a.sample_stats + pair);
                }
                wave_sync_lds();  // wh is zeroed again for the wave's next pair
            }
            __syncthreads();
            for (uint32_t b = tid; b < ids.bins; b += blockDim.x) {
                if (hb[b]) atomicAdd((unsigned long long*)&a.hist[out_bins + b], hb[b]);
                if (SHIST_LDS && sampling && hbs[b]) atomicAdd((unsigned long long*)&a.sample_hist[out_bins + b], hbs[b]);
            }
            __syncthreads();
        }
        r = seg_end;
    }
}

}  // namespace

hipError_t launch_snapstats(const SnapStatsArgs& a, uint32_t blocks, hipStream_t stream) {
    SnapStatsArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    bool in_lds = false;
    const uint32_t nw = snapstats_waves(a.ids.bins, a.table_slots, &lds, &in_lds);
    if (lds > kPassLdsMax) return hipErrorInvalidValue;
    const void* fn = in_lds ? (const void*)ssa_snapstats<true> : (const void*)ssa_snapstats<false>;
    return hipLaunchKernel(fn, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
