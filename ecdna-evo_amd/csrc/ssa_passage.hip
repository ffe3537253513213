// ssa_passage.hip — the phase boundary of a serial-passage run (ecdna_ssa_passages_t; gfx950).
//
// The reference's cell-line strategy restarts growth from the subsample: a culture is grown, a few hundred cells are
// taken and measured, and those same cells found the next flask. At the end of growth phase g this pass draws each
// replicate's sample of m cells by subsample mapping v1 under the phase's key seed_g (include/ecdna_ssa.h, DESIGN.md
// §3.4), writes the sample's ecdna_rep_stats_t and the per-set sum of the samples' histograms exactly as
// ssa_subsample.hip does (the phase's "measurement"), and, unless the phase is the last, materialises the sample as
// the founders of phase g + 1: {n-, n+} per replicate and the n+ true copy numbers in ascending order, which is the
// order an initial histogram gives the steppers' replicate start.
//
// One wave per replicate. Per wave in LDS: the replicate's histogram wh (u32 per bin), the inclusive prefix sums of its
// bin counters pre (position -> copy number), the table of drawn positions tab, and the founders fs (u16, a power of
// two >= 64 slots padded with 0xffff for the sort). The draws, the table and the lookup are ssa_sampledraw.hpp's.
//  - sample = the picks (m' = m): every new pick of an N+ position appends its copy number (wave_sample_picks).
//  - complement (m' = N - m, so N <= 2m): the positions are walked once, those not in the table are the sample.
//  - m >= N: every position.
// The founders are then ordered by a bitonic sort of the wave over the first pow2ceil(n+) slots. A sample the guard
// ended (all-zero statistics) founds the empty population, as does an empty one.
// The samples' non-zero bins go to global memory directly: a workgroup histogram beside 2,048 bins and m = 4096 would
// not fit 64 KiB of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

constexpr uint32_t kPasBlock = 256;
constexpr uint32_t kPasPad = 0xffffu;

// fs[0 .. P) ascending, P a power of two >= 64: the wave's bitonic network, 64 compare-exchanges per step.
__device__ __forceinline__ void wave_bitonic_sort_u16(uint16_t* fs, uint32_t P, uint32_t lane) {
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint16_t x = fs[i], y = fs[l];
                    const bool up = (i & k) == 0u;
                    if ((x > y) == up) {
                        fs[i] = y;
                        fs[l] = x;
                    }
                }
            }
            wave_sync_lds();
        }
    }
}

// BAG as in ssa_hist: 0 = rows only; 1 / 2 = u16 / u32 bin counters bags[q][bag_k] for copy numbers 1..bag_k plus
// the large-k cells at the head of the row.
template <int BAG>
__global__ void __launch_bounds__(kPasBlock) ssa_passage(const PassageArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t wave_words = a.bins + a.bag_k + a.table_slots + (a.sort_slots >> 1);
    uint32_t* wh = lds + (size_t)wave * wave_words;              // [bins]
    uint32_t* pre = wh + a.bins;                                 // [bag_k]
    uint32_t* tab = pre + a.bag_k;                               // [table_slots]
    uint16_t* fs = reinterpret_cast<uint16_t*>(tab + a.table_slots);  // [sort_slots]
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);
    const uint32_t last = a.bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const bool want = a.founder_rows != nullptr;
    const uint32_t fcap = min(a.m, a.sort_slots);  // a founder row is never written past m

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const ecdna_rep_summary_t* s = a.summaries + q;
        const uint64_t nm = s->nminus;
        const uint32_t np = (uint32_t)s->nplus;
        const uint64_t cells_all = nm + (uint64_t)np;
        const uint64_t rid = a.rid0 + (uint64_t)q * a.rid_stride;
        const uint64_t set = rid / a.reps_per_set;
        const uint16_t* row = a.rows + (uint64_t)q * a.row_stride;
        // the sample is the whole population (m >= N), the picked positions (m' = m) or what they leave (m' < m)
        const bool whole = (uint64_t)a.m >= cells_all;
        bool bad = !whole && cells_all >= 0xffffffffull;  // positions are u32, 0xffffffff marks an empty slot
        const uint32_t N = (uint32_t)cells_all;
        const uint32_t mp = (whole || bad) ? 0u : min(a.m, N - a.m);
        const bool comp = mp != a.m;
        const bool need_full = whole || comp;
        for (uint32_t b = lane; b < a.bins; b += 64u) wh[b] = 0u;
        if (want)
            for (uint32_t b = lane; b < a.sort_slots; b += 64u) fs[b] = (uint16_t)kPasPad;
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

        // 2.-4. draws until m' distinct positions have appeared; every new one is looked up and counted (and, when the
        // picks are the sample, gathered as a founder)
        const SamplePop pop{nm, pre, a.bag_k, small, row, nrow};
        uint64_t psum = 0;  // sum of k over the picked positions
        uint32_t gn = 0;    // founders gathered (N+ cells)
        if (!whole && !bad)
            bad = wave_sample_picks<BAG>(wh, tab, a.table_slots, pop, N, mp, comp, last, sample_stream_tag(0u), rid, k0,
                                         k1, lane, psum, want ? fs : nullptr, fcap, &gn);
        wave_sync_lds();

        // founders of a whole population or of a complement: one walk over the positions (N <= 2m), from the 64-block
        // that holds the first N+ position on
        bool fbad = bad;
        if (want && !bad && need_full) {
            const SampleTable tb = sample_table(mp);
            bool lane_bad = false;
            for (uint32_t base = (uint32_t)min(nm, (uint64_t)N) & ~63u; base < N; base += 64u) {
                const uint32_t v = base + lane;
                bool keep = v < N && (whole || !sample_tab_has(tab, tb, v));
                uint32_t kk = 0;
                if (keep && !sample_pos_k<BAG>(pop, v, kk)) {
                    lane_bad = true;
                    keep = false;
                }
                wave_append_u16(keep && kk > 0u, kk, fs, fcap, gn, lane);
            }
            fbad = __any(lane_bad);
            wave_sync_lds();
        }

        // 5. statistics of the sample histogram (the guard, or a state the counters cannot account for: all-zero
        // sample statistics, nothing added to the sample histogram)
        ksum = wave_sum(ksum);
        psum = wave_sum(psum);
        const uint32_t nminus_s = wh[0];  // the sample's N- cells (whole: all of them; complement: those left)
        if (bad) {
            if (lane == 0) a.stats[q] = ecdna_rep_stats_t{};
        } else {
            const uint64_t cells = whole ? cells_all : (uint64_t)a.m;
            const uint64_t ks_sum = whole ? ksum : (comp ? ksum - psum : psum);
            const uint64_t nplus_s = whole ? (uint64_t)np : cells - (uint64_t)nminus_s;
            wave_rep_stats(wh, reinterpret_cast<unsigned long long*>(a.sample_hist + set * a.bins), a.bins, cells, ks_sum,
                           nplus_s, a.has_target, a.target_cdf, a.target_mean, a.target_entropy, a.target_freq, lane,
                           a.stats + q);
        }

        // 6. the founders, ascending
        if (want) {
            if (fbad || gn > fcap) gn = 0;  // (gn > fcap: more N+ cells than a sample holds, unreachable)
            if (gn > 1u) {
                uint32_t P = 64u;
                while (P < gn) P <<= 1;
                wave_bitonic_sort_u16(fs, P, lane);
            }
            uint16_t* out = a.founder_rows + (uint64_t)q * a.founder_stride;
            for (uint32_t j = lane; j < gn; j += 64u) out[j] = fs[j];
            if (lane == 0) a.founder_counts[q] = make_uint2(fbad ? 0u : nminus_s, gn);
        }
        wave_sync_lds();  // wh and fs are reset for the wave's next replicate
    }
}

}  // namespace

uint32_t passage_sort_slots(uint32_t m) {
    uint32_t p = 64;
    while (p < m) p <<= 1;
    return p;
}

uint32_t passage_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, uint32_t sort_slots, size_t* lds_bytes) {
    // 1, 2 or 4 waves per workgroup, as many as keep the workgroup within 64 KiB of dynamic LDS
    for (uint32_t nw = kPasBlock / 64u; nw >= 1u; nw >>= 1) {
        const size_t lds = (size_t)nw * ((size_t)bins + bag_k + table_slots + (sort_slots >> 1)) * sizeof(uint32_t);
        if (lds <= 65536u || nw == 1u) {
            if (lds_bytes) *lds_bytes = lds;
            return nw;
        }
    }
    return 1u;
}

hipError_t launch_passage(const PassageArgs& a, uint32_t blocks, hipStream_t stream) {
    PassageArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = passage_waves(a.bins, a.bag_k, a.table_slots, a.sort_slots, &lds);
    if (lds > 65536u || a.m > a.founder_stride || a.sort_slots < 64u || (a.sort_slots & (a.sort_slots - 1u)))
        return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_passage<0>, (const void*)ssa_passage<1>,
                                         (const void*)ssa_passage<2>};
    const int bag = a.bags ? (a.bag_c32 ? 2 : 1) : 0;
    return hipLaunchKernel(table[bag], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
