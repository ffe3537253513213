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
// position -> copy number lookup are wave_sample_picks (ssa_sampledraw.hpp), shared with ssa_snapstats.hip.
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
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t wave_words = a.bins + a.bag_k + a.table_slots;
    uint32_t* wh = reinterpret_cast<uint32_t*>(lds + a.bins) + (size_t)wave * wave_words;  // [bins]
    uint32_t* pre = wh + a.bins;                                                           // [bag_k]
    uint32_t* tab = pre + a.bag_k;                                                         // [table_slots]
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);
    const uint32_t last = a.bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    uint32_t r = r_begin;
    while (r < r_end) {
        const auto [set, seg_end] = set_segment(a.rid0, a.rid_stride, a.reps_per_set, r, r_end);
        for (uint32_t b = tid; b < a.bins; b += blockDim.x) hb[b] = 0ull;
        __syncthreads();
        for (uint32_t q = r + wave; q < seg_end; q += nw) {
            const ecdna_rep_summary_t* s = a.summaries + q;
            const uint64_t nm = s->nminus;
            const uint32_t np = (uint32_t)s->nplus;
            const uint64_t cells_all = nm + (uint64_t)np;
            const uint64_t rid = a.rid0 + (uint64_t)q * a.rid_stride;
            const uint16_t* row = a.rows + (uint64_t)q * a.row_stride;
            // the sample is the whole population (m >= N), the picked positions (m' = m) or what they leave (m' < m)
            const bool whole = (uint64_t)a.m >= cells_all;
            bool bad = !whole && cells_all >= 0xffffffffull;  // positions are u32, 0xffffffff marks an empty slot
            const uint32_t N = (uint32_t)cells_all;
            const uint32_t mp = (whole || bad) ? 0u : min(a.m, N - a.m);
            const bool comp = mp != a.m;
            const bool need_full = whole || comp;
            for (uint32_t b = lane; b < a.bins; b += 64u) wh[b] = 0u;
            wave_sync_lds();

            // 1. counters: prefix sums for the position -> k lookup, and (whole / complement) the full histogram
            uint64_t ksum = 0;  // sum of k over the full population (need_full)
            uint32_t small = 0;
            if (BAG) {
                for (uint32_t base = 0; base < a.bag_k; base += 64u) {
                    const uint32_t b = base + lane;
                    const uint32_t cnt = b < a.bag_k ? bag_counter<BAG>(a.bags, q, a.bag_k, b) : 0u;
                    if (need_full && cnt) {
                        const uint32_t kk = b + 1u;
                        atomicAdd(&wh[kk < last ? kk : last], cnt);
                        ksum += (uint64_t)kk * cnt;
                    }
                    const uint32_t scan = wave_inclusive_scan(cnt, lane);
                    if (b < a.bag_k) pre[b] = small + scan;
                    small += __shfl(scan, 63, 64);
                }
                if (!whole && small > np) bad = true;  // the counters hold more cells than the summary
            }
            // cells held in the row (never trust counters past the row, nor the summary past the row's memory)
            const uint32_t nrow = (uint32_t)min((uint64_t)(np >= small ? np - small : 0u), a.row_stride);
            if (need_full) {
                for (uint32_t c = lane * 8u; c < nrow; c += 512u) {
                    const uint4 v = *reinterpret_cast<const uint4*>(row + c);
                    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (c + (uint32_t)j < nrow) {
                            const uint32_t kk = (wv[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                            atomicAdd(&wh[kk < last ? kk : last], 1u);
                            ksum += kk;
                        }
                    }
                }
                if (lane == 0) atomicAdd(&wh[0], (uint32_t)nm);
            }

            // 2.-4. draws until m' distinct positions have appeared; every new one is looked up and counted
            uint64_t psum = 0;  // sum of k over the picked positions
            if (!whole && !bad) {
                const SamplePop pop{nm, pre, a.bag_k, small, row, nrow};
                bad = wave_sample_picks<BAG>(wh, tab, a.table_slots, pop, N, mp, comp, last, sample_stream_tag(0u), rid,
                                             k0, k1, lane, psum);
            }
            wave_sync_lds();

            // 5. statistics of the sample histogram (the guard, or a state the counters cannot account for: all-zero
            // sample statistics, nothing added to hb)
            ksum = wave_sum(ksum);
            psum = wave_sum(psum);
            if (bad) {
                if (lane == 0) a.stats[q] = ecdna_rep_stats_t{};
            } else {
                const uint64_t cells = whole ? cells_all : (uint64_t)a.m;
                const uint64_t ks_sum = whole ? ksum : (comp ? ksum - psum : psum);
                const uint64_t nplus_s = whole ? (uint64_t)np : cells - (uint64_t)wh[0];
                wave_rep_stats(wh, hb, a.bins, cells, ks_sum, nplus_s, a.has_target, a.target_cdf, a.target_mean,
                               a.target_entropy, a.target_freq, lane, a.stats + q);
            }
            wave_sync_lds();  // wh is zeroed again for the wave's next replicate
        }
        __syncthreads();
        for (uint32_t b = tid; b < a.bins; b += blockDim.x)
            if (hb[b]) atomicAdd((unsigned long long*)&a.sample_hist[set * a.bins + b], hb[b]);
        __syncthreads();
        r = seg_end;
    }
}

}  // namespace

uint32_t subsample_table_slots(uint32_t m) {
    uint32_t p = 1;
    while (p < m) p <<= 1;
    return 2u * p;
}

uint32_t subsample_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, size_t* lds_bytes) {
    // 1, 2 or 4 waves per workgroup, as many as keep the workgroup within 64 KiB of dynamic LDS
    for (uint32_t nw = kSubBlock / 64u; nw >= 1u; nw >>= 1) {
        const size_t lds = (size_t)bins * sizeof(unsigned long long) +
                           (size_t)nw * ((size_t)bins + bag_k + table_slots) * sizeof(uint32_t);
        if (lds <= 65536u || nw == 1u) {
            if (lds_bytes) *lds_bytes = lds;
            return nw;
        }
    }
    return 1u;
}

hipError_t launch_subsample(const SubsampleArgs& a, uint32_t blocks, hipStream_t stream) {
    SubsampleArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = subsample_waves(a.bins, a.bag_k, a.table_slots, &lds);
    if (lds > 65536u) return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_subsample<0>, (const void*)ssa_subsample<1>,
                                         (const void*)ssa_subsample<2>};
    const int bag = a.bags ? (a.bag_c32 ? 2 : 1) : 0;
    return hipLaunchKernel(table[bag], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
