// ssa_subsample.hip — end-of-run subsampling fused with the per-replicate ABC statistics (gfx950).
//
// The reference ends every run with into_subsampled(nb, &mut rng) (src/main.rs:110-123, 184-197): a patient's
// data is a sample of some hundreds of cells, never the whole tumour, and the statistics an ABC caller compares
// are those of the sample. This pass draws each replicate's sample of subsample_cells cells from its final
// state where that state already lies (bin counters in `bags`, large-k cells in `rows`), right after ssa_hist
// and on the same stream, and writes the sample's ecdna_rep_stats_t and the per-set sum of the samples'
// histograms. The sample's law is subsample mapping v1 (include/ecdna_ssa.h);
// tests/subsample_law.py restates it in numpy.
//
// One wave per replicate, as ssa_hist<true, BAG>. Per wave in LDS: the replicate's histogram (u32 per bin), the
// inclusive prefix sums of its bin counters (position -> copy number), and an open-addressing table of the
// positions drawn so far (u32, 0xffffffff = empty), which decides whether a draw is new. The draws, the table and the
// position -> copy number lookup, and the steps around them that ssa_passage.hip takes too, are ssa_sampledraw.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

constexpr uint32_t kSubBlock = 256;

// BAG as in ssa_hist: 0 = rows only; 1 / 2 = u16 / u32 bin counters bags[q][bag_k] for copy numbers 1..bag_k plus
// the large-k cells at the head of the row.
template <int BAG>
__global__ void __launch_bounds__(kSubBlock) ssa_subsample(const SubsampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    unsigned long long* hb = lds;  // [bins] the workgroup's sum of sample histograms (one parameter set at a time)
    const ChunkIds& ids = a.ids;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t wave_words = ids.bins + a.state.bag_k + a.table_slots;
    uint32_t* wh = reinterpret_cast<uint32_t*>(lds + ids.bins) + (size_t)wave * wave_words;  // [bins]
    uint32_t* pre = wh + ids.bins;                                                           // [bag_k]
    uint32_t* tab = pre + a.state.bag_k;                                                        // [table_slots]
    const uint32_t r_begin = blockIdx.x * ids.reps_per_block;
    if (r_begin >= ids.n) return;
    const uint32_t r_end = min(ids.n, r_begin + ids.reps_per_block);
    const uint32_t last = ids.bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    uint32_t r = r_begin;
    while (r < r_end) {
        const auto [set, seg_end] = set_segment(ids.rid0, ids.rid_stride, ids.reps_per_set, r, r_end);
        for (uint32_t b = tid; b < ids.bins; b += blockDim.x) hb[b] = 0ull;
        __syncthreads();
        for (uint32_t q = r + wave; q < seg_end; q += nw) {
            const ecdna_rep_summary_t* s = a.state.summaries + q;
            const uint64_t nm = s->nminus;
            const uint32_t np = (uint32_t)s->nplus;
            const uint64_t rid = ids.rid0 + (uint64_t)q * ids.rid_stride;
            SamplePlan plan = sample_plan(a.m, nm + (uint64_t)np);

            // 1. counters: prefix sums for the position -> k lookup, and (whole / complement) the full histogram
            uint64_t ksum = 0;  // sum of k over the full population (need_full)
            const SamplePop pop = wave_load_final_state<BAG>(a.state, q, nm, np, ids.bins, plan, wh, pre, ksum, lane);

            // 2.-4. draws until m' distinct positions have appeared; every new one is looked up and counted
            uint64_t psum = 0;  // sum of k over the picked positions
            bool bad = plan.bad;
            if (!plan.whole && !bad)
                bad = wave_sample_picks<BAG>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                             sample_stream_tag(0u), rid, k0, k1, lane, psum);
            wave_sync_lds();

            // 5. statistics of the sample histogram, its bins added to hb
            wave_sample_stats(plan, bad, a.m, nm + (uint64_t)np, np, ksum, psum, wh, hb, ids.bins, a.target, lane,
                              a.stats + q);
            wave_sync_lds();  // wh is zeroed again for the wave's next replicate
        }
        __syncthreads();
        for (uint32_t b = tid; b < ids.bins; b += blockDim.x)
            if (hb[b]) atomicAdd((unsigned long long*)&a.sample_hist[set * ids.bins + b], hb[b]);
        __syncthreads();
        r = seg_end;
    }
}

}  // namespace

hipError_t launch_subsample(const SubsampleArgs& a, uint32_t blocks, hipStream_t stream) {
    SubsampleArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = subsample_waves(a.ids.bins, a.state.bag_k, a.table_slots, &lds);
    if (lds > kPassLdsMax) return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_subsample<0>, (const void*)ssa_subsample<1>,
                                         (const void*)ssa_subsample<2>};
    return hipLaunchKernel(table[bag_index(a.state)], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
