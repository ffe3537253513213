// ssa_rescore.hip — the passes over the kept samples of a run (ecdna_ssa_keep_t, keep mapping v1, include/ecdna_ssa.h;
// DESIGN.md §3.4; gfx950): late scoring, the posterior predictive histogram, and the gather of listed samples.
//
// A kept sample is {n-, n+} and the n+ true copy numbers, ascending (written by ssa_passage's KEEP instance). A record
// is a pure function of the sample's clipped histogram, its true sum of k and its size, so the record ssa_rescore makes
// from the kept cells is byte for byte the one the launch-time passes make from the final state: the histogram and the
// sums are integers, and the f64 operations on them are wave_cohort_stats' (ssa_wave.hpp), the routine ssa_cohort.hip
// scores with, in its lane and scan order (fp contract off).
//
//  - ssa_rescore: one wave per replicate over the whole run. The wave reads the header and the n+ cells, builds the
//    clipped histogram in LDS (wh[0] = n-), sums the true copy numbers and scores against all P targets; lane p writes
//    record [p][i]. A header the guard left gives all-zero records. Per wave in LDS: wh (u32 per bin) and the CDF (f64
//    per bin); no workgroup state and no workgroup barrier.
//  - ssa_pool_accepted: a workgroup walks its replicates by parameter-set segment, as ssa_subsample does. A wave reads
//    64 replicates' mask words with one load; the accepted ones' cells are counted into the workgroup's u64 histogram in
//    LDS, and one u64 atomic per non-zero bin flushes it to the set's row. An unaccepted replicate costs its mask read.
//  - ssa_kept_gather: one wave per listed replicate copies the header and the m cells.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_launch.h"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

__global__ void __launch_bounds__(256) ssa_rescore(const RescoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = a.bins, last = bins - 1u;
    // (the CDFs first: every wave's is 8-byte aligned whatever the parity of bins)
    double* F = reinterpret_cast<double*>(lds) + (size_t)wave * bins;                            // [bins]
    uint32_t* wh = reinterpret_cast<uint32_t*>(lds + (size_t)nw * bins) + (size_t)wave * bins;  // [bins]
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint2 h = a.headers[q];
        if (h.x == kKeptGuard && h.y == kKeptGuard) {  // the guard: all-zero statistics, as wave_sample_stats
            if (lane < a.n_targets) a.out[q + (uint64_t)lane * a.n] = ecdna_rep_stats_t{};
            continue;
        }
        const uint32_t np = min(h.y, a.m);  // (a row holds m cells)
        for (uint32_t b = lane; b < bins; b += 64u) wh[b] = 0u;
        wave_sync_lds();
        const uint16_t* row = a.cells + (uint64_t)q * a.m;
        uint64_t ksum = 0;
        for (uint32_t j = lane; j < np; j += 64u) {
            const uint32_t kk = row[j];
            atomicAdd(&wh[kk < last ? kk : last], 1u);
            ksum += kk;
        }
        if (lane == 0) atomicAdd(&wh[0], h.x);
        wave_sync_lds();
        ksum = wave_sum(ksum);
        wave_cohort_stats(wh, F, bins, (uint64_t)h.x + np, ksum, np, a.target_cdf, a.target_scalars, nullptr,
                          a.n_targets, lane, a.out + q, a.n);
        wave_sync_lds();  // wh and the CDF are written again for the wave's next replicate
    }
}

__global__ void __launch_bounds__(kPoolBlock) ssa_pool_accepted(const PoolAcceptedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hb[];  // [bins]: one parameter set at a time
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = a.bins, last = bins - 1u;
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);

    uint32_t r = r_begin;
    while (r < r_end) {
        const auto [set, seg_end] = set_segment(a.rid0, a.rid_stride, a.reps_per_set, r, r_end);
        for (uint32_t b = tid; b < bins; b += blockDim.x) hb[b] = 0ull;
        __syncthreads();
        bool any = false;
        for (uint32_t base = r + wave * 64u; base < seg_end; base += nw * 64u) {
            const uint32_t mine = base + lane;
            const bool acc = mine < seg_end && ((a.mask[mine] >> a.q) & 1u);
            unsigned long long todo = __ballot(acc);
            while (todo) {
                const uint32_t q = base + (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1ull;
                const uint2 h = a.headers[q];
                if (h.x == kKeptGuard && h.y == kKeptGuard) continue;  // the guard: adds nothing
                const uint32_t np = min(h.y, a.m);
                const uint16_t* row = a.cells + (uint64_t)q * a.m;
                for (uint32_t j = lane; j < np; j += 64u) {
                    const uint32_t kk = row[j];
                    atomicAdd(&hb[kk < last ? kk : last], 1ull);
                }
                if (lane == 0 && h.x) atomicAdd(&hb[0], (unsigned long long)h.x);
                any = true;
            }
        }
        // (a segment that accepted nothing is not flushed: every lane of a wave holds the same `any`)
        const bool flush = __syncthreads_or(any);
        if (flush)
            for (uint32_t b = tid; b < bins; b += blockDim.x)
                if (hb[b]) atomicAdd(&a.hist[set * bins + b], hb[b]);
        __syncthreads();
        r = seg_end;
    }
}

__global__ void __launch_bounds__(kGatherBlock) ssa_kept_gather(const KeptGatherArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= a.n_ids) return;
    const uint32_t q = a.index[j];
    if (lane == 0) a.out_headers[j] = a.headers[q];
    const uint16_t* src = a.cells + (uint64_t)q * a.m;
    uint16_t* dst = a.out_cells + (uint64_t)j * a.m;
    for (uint32_t x = lane; x < a.m; x += 64u) dst[x] = src[x];
}

}  // namespace

hipError_t launch_rescore(const RescoreArgs& a, hipStream_t stream) {
    RescoreArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = rescore_waves(a.bins, &lds);
    if (lds > kPassLdsMax || a.n_targets < 1u || a.n_targets > kMaxCohortTargets || !a.n || !a.reps_per_block ||
        a.bins < 2u)
        return hipErrorInvalidValue;
    const uint32_t blocks = (a.n + a.reps_per_block - 1u) / a.reps_per_block;
    return hipLaunchKernel((const void*)ssa_rescore, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

hipError_t launch_pool_accepted(const PoolAcceptedArgs& a, hipStream_t stream) {
    PoolAcceptedArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = pool_accepted_waves(a.bins, &lds);
    if (lds > kPassLdsMax || a.q >= kMaxAcceptRows || !a.n || !a.reps_per_block || a.bins < 2u || !a.rid_stride)
        return hipErrorInvalidValue;
    const uint32_t blocks = (a.n + a.reps_per_block - 1u) / a.reps_per_block;
    return hipLaunchKernel((const void*)ssa_pool_accepted, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

hipError_t launch_kept_gather(const KeptGatherArgs& a, hipStream_t stream) {
    KeptGatherArgs copy = a;
    void* args[] = {&copy};
    if (!a.n_ids) return hipErrorInvalidValue;
    const uint32_t per_block = (uint32_t)kGatherBlock / 64u;
    return hipLaunchKernel((const void*)ssa_kept_gather, dim3((a.n_ids + per_block - 1u) / per_block),
                           dim3(kGatherBlock), args, 0, stream);
}

}  // namespace ecdna
