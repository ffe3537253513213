// ssa_accept.hip — ABC rejection on the GPU (gfx950): the acceptance pass of ecdna_ssa_ctx_accept over statistics the
// context already holds (acceptance mapping v1, include/ecdna_ssa.h).
//
// The statistics of a run stay in HBM after a launch; this pass turns them into what a rejection sampler keeps: per
// replicate a 32-bit mask (bit q = accepted under threshold row q), per row and parameter set the number accepted (the
// posterior's counts), and for one row the ordered list of the accepted replicates with their records. It runs over the
// whole run at once (the statistics buffers are sized by the run, not the chunk) and as often as the caller likes after
// one launch.
//
// ssa_accept_mask: one lane per replicate. The lane reads its error words and the four distances of its participating
// records, tests them against every row (the thresholds lie in the argument block: scalar loads) and stores its mask.
// For the counts the wave walks its parameter-set segments (set_segment), ballots each row inside the segment, and
// lane q adds row q's popcount with one u64 atomic per (wave, set, row) that accepted anything: integer adds, exact in
// any order.
//
// The list is an ordered stream compaction in three launches — ssa_accept_block_counts (accepted per workgroup),
// ssa_accept_scan (their exclusive prefix sums, one workgroup), ssa_accept_scatter (ids and records to their places
// by the wave's ballot and prefix popcount) — so the order is that of the replicates whatever the scheduling, and no
// workgroup ever waits for another. Entries at or past list_capacity are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_launch.h"
#include "ssa_wave.hpp"

namespace ecdna {

namespace {

constexpr uint32_t kAcceptWaves = kAcceptBlock / 64;
constexpr int kScanBlock = 1024;

// A distance passes a threshold it does not exceed (a tie passes); +inf switches the statistic off, NaN distances
// included; a NaN distance fails every finite threshold.
__device__ __forceinline__ bool passes(double d, double thr) { return thr == __builtin_huge_val() || d <= thr; }

__global__ void __launch_bounds__(kAcceptBlock) ssa_accept_mask(const AcceptArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t at = (uint64_t)blockIdx.x * kAcceptBlock + tid;
    const bool live = at < a.n;
    const uint32_t i = (uint32_t)at;
    uint32_t m = 0u;
    if (live) {
        uint32_t err = 0u;
        if (a.err_stride == 0u) {
            err = a.summaries[i].error;
        } else {
            for (uint32_t t = 0; t < a.T; ++t)
                if ((a.tmask >> t) & 1ull) err |= a.summaries[(uint64_t)i + t * a.err_stride].error;
        }
        if (!err) {
            m = a.Q >= 32u ? 0xffffffffu : (1u << a.Q) - 1u;
            for (uint32_t t = 0; t < a.T; ++t) {
                if (!((a.tmask >> t) & 1ull)) continue;
                const ecdna_rep_stats_t* rec = a.stats + ((uint64_t)i * a.rep_stride + t * a.tp_stride);
                const double ks = rec->ks, mean_rel = rec->mean_rel, entropy_rel = rec->entropy_rel,
                             frequency_diff = rec->frequency_diff;
                for (uint32_t q = 0; q < a.Q; ++q) {
                    const bool ok = passes(ks, a.thr[q][0]) && passes(mean_rel, a.thr[q][1]) &&
                                    passes(entropy_rel, a.thr[q][2]) && passes(frequency_diff, a.thr[q][3]);
                    if (!ok) m &= ~(1u << q);
                }
            }
        }
        a.mask[i] = m;
    }

    // the counts: per parameter-set segment of the wave, row q's ballot; lane q adds its popcount
    const uint64_t wave_base = at - lane;
    if (wave_base >= a.n) return;
    const uint32_t r_end = (uint32_t)min((uint64_t)a.n, wave_base + 64u);
    uint32_t r = (uint32_t)wave_base;
    while (r < r_end) {
        const auto [set, seg_end] = set_segment(a.rid0, a.rid_stride, a.reps_per_set, r, r_end);
        const bool in_seg = live && i >= r && i < seg_end;
        uint32_t mine = 0u;
        for (uint32_t q = 0; q < a.Q; ++q) {
            const unsigned long long b = __ballot(in_seg && ((m >> q) & 1u));
            if (lane == q) mine = (uint32_t)__popcll(b);
        }
        if (mine) atomicAdd(&a.counts[(uint64_t)lane * a.n_sets + set], (unsigned long long)mine);
        r = seg_end;
    }
}

// The lane's replicate is accepted under the list's row; its ballot over the wave.
__device__ __forceinline__ bool listed(const AcceptArgs& a, uint64_t at) {
    return at < a.n && ((a.mask[at] >> a.list_q) & 1u);
}

__global__ void __launch_bounds__(kAcceptBlock) ssa_accept_block_counts(const AcceptArgs a) {
    __shared__ uint32_t wave_count[kAcceptWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned long long b = __ballot(listed(a, (uint64_t)blockIdx.x * kAcceptBlock + tid));
    if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (tid == 0u) {
        uint32_t total = 0u;
        for (uint32_t w = 0; w < kAcceptWaves; ++w) total += wave_count[w];
        a.block_counts[blockIdx.x] = total;
    }
}

// block_counts[b] becomes the number accepted in the workgroups before b. One workgroup walks the array kScanBlock
// entries at a time with the running total in a register (the totals stay below n < 2^32).
__global__ void __launch_bounds__(kScanBlock) ssa_accept_scan(uint32_t* block_counts, uint32_t n_blocks) {
    __shared__ uint32_t wave_total[kScanBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < n_blocks; base += kScanBlock) {
        const uint32_t idx = base + tid;
        const uint32_t v = idx < n_blocks ? block_counts[idx] : 0u;
        const uint32_t incl = wave_inclusive_scan(v, lane);
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < kScanBlock / 64; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (idx < n_blocks) block_counts[idx] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kAcceptBlock) ssa_accept_scatter(const AcceptArgs a) {
    __shared__ uint32_t wave_count[kAcceptWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t at = (uint64_t)blockIdx.x * kAcceptBlock + tid;
    const bool acc = listed(a, at);
    const unsigned long long b = __ballot(acc);
    if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint64_t pos = a.block_counts[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) pos += wave_count[w];
    pos += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (!acc || pos >= a.list_capacity) return;
    a.ids[pos] = a.rid0 + at * a.rid_stride;
    for (uint32_t t = 0; t < a.T; ++t) {  // 64-byte records, 64-byte aligned
        const uint4* src = reinterpret_cast<const uint4*>(a.stats + (at * a.rep_stride + t * a.tp_stride));
        uint4* dst = reinterpret_cast<uint4*>(a.list_stats + (pos * a.T + t));
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = src[k];
    }
}

}  // namespace

hipError_t launch_accept_mask(const AcceptArgs& a, hipStream_t stream) {
    AcceptArgs copy = a;
    void* args[] = {&copy};
    return hipLaunchKernel((const void*)ssa_accept_mask, dim3(a.n_blocks), dim3(kAcceptBlock), args, 0, stream);
}

hipError_t launch_accept_list(const AcceptArgs& a, hipStream_t stream) {
    AcceptArgs copy = a;
    void* args[] = {&copy};
    hipError_t e =
        hipLaunchKernel((const void*)ssa_accept_block_counts, dim3(a.n_blocks), dim3(kAcceptBlock), args, 0, stream);
    if (e != hipSuccess) return e;
    uint32_t* bc = a.block_counts;
    uint32_t nb = a.n_blocks;
    void* scan_args[] = {&bc, &nb};
    e = hipLaunchKernel((const void*)ssa_accept_scan, dim3(1), dim3(kScanBlock), scan_args, 0, stream);
    if (e != hipSuccess) return e;
    return hipLaunchKernel((const void*)ssa_accept_scatter, dim3(a.n_blocks), dim3(kAcceptBlock), args, 0, stream);
}

}  // namespace ecdna
