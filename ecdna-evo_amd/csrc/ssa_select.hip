// ssa_select.hip — ABC thresholds on the GPU (gfx950): the device side of ecdna_ssa_ctx_select and
// ecdna_ssa_ctx_select_digits (select mapping v1, include/ecdna_ssa.h), an 8-bit radix select over the statistics the
// context already holds. Each pass leaves a small integer histogram; the host walks it to the next prefix
// (ssa_select.hpp), and shards' histograms sum exactly.
//
// ssa_select_keys: one lane per replicate, once per (source, timepoint mask). The lane reads its error words and the
// four distances of its participating records as ssa_accept_mask does, and stores per distance the maximum of their
// keys (select::key_of, the function the CPU check calls) into keys[4][n], or select::kExcluded for a replicate with an
// error. The passes then read 8 coalesced bytes per replicate and distance instead of T strided 64-byte records: with
// T = 64 a pass over the records would read 4 KiB per replicate eight times over.
//
// ssa_select_digits: blockIdx.y is the distance, and a workgroup walks reps_per_block consecutive replicates, 256 at a
// time, not one lane per replicate: a workgroup of 256 replicates would add up to 256 counters to the global histogram,
// as many atomics as with no LDS table at all. The pass's distinct prefixes travel in the argument block (scalar
// loads); a lane whose key has one of them in its top bits bumps a u32 counter of the LDS table [groups][256]. Keys of
// one distance often share their top bytes, so the wave first adds the popcount of the lanes that share the first
// lane's counter with one atomic, and only the others add 1 each. At the end the workgroup adds its non-zero counters
// to the global u64 histogram: integer atomics, exact in any order. No workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_launch.h"
#include "ssa_select.hpp"

namespace ecdna {

namespace {

constexpr uint32_t kNoSlot = 0xffffffffu;

__global__ void __launch_bounds__(kSelectBlock) ssa_select_keys(const SelectKeyArgs a) {
    const uint64_t at = (uint64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    if (at >= a.n) return;
    const uint32_t i = (uint32_t)at;
    uint32_t err = 0u;
    if (a.err_stride == 0u) {
        err = a.summaries[i].error;
    } else {
        for (uint32_t t = 0; t < a.T; ++t)
            if ((a.tmask >> t) & 1ull) err |= a.summaries[(uint64_t)i + t * a.err_stride].error;
    }
    uint64_t k0 = select::kExcluded, k1 = select::kExcluded, k2 = select::kExcluded, k3 = select::kExcluded;
    if (!err) {
        k0 = k1 = k2 = k3 = 0ull;
        for (uint32_t t = 0; t < a.T; ++t) {
            if (!((a.tmask >> t) & 1ull)) continue;
            const ecdna_rep_stats_t* rec = a.stats + ((uint64_t)i * a.rep_stride + t * a.tp_stride);
            k0 = max(k0, select::key_of(rec->ks));
            k1 = max(k1, select::key_of(rec->mean_rel));
            k2 = max(k2, select::key_of(rec->entropy_rel));
            k3 = max(k3, select::key_of(rec->frequency_diff));
        }
    }
    a.keys[at] = k0;
    a.keys[(uint64_t)a.n + at] = k1;
    a.keys[2ull * a.n + at] = k2;
    a.keys[3ull * a.n + at] = k3;
}

__global__ void __launch_bounds__(kSelectBlock) ssa_select_digits(const SelectArgs a) {
    extern __shared__ uint32_t table[];  // [n_groups[x]][256]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, x = blockIdx.y;
    const uint32_t G = a.n_groups[x];
    const uint32_t slots = G * select::kDigits;
    for (uint32_t s = tid; s < slots; s += kSelectBlock) table[s] = 0u;
    __syncthreads();

    const uint64_t* keys = a.keys + (uint64_t)x * a.n;
    const uint64_t begin = (uint64_t)blockIdx.x * a.reps_per_block;
    const uint64_t end = min((uint64_t)a.n, begin + a.reps_per_block);
    for (uint64_t base = begin; base < end; base += kSelectBlock) {
        const uint64_t at = base + tid;
        uint32_t slot = kNoSlot;
        if (at < end) {
            const uint64_t key = keys[at];
            if (key != select::kExcluded) {
                const uint64_t top = select::key_top(key, a.pass);
                const uint32_t digit = select::key_digit(key, a.pass);
                for (uint32_t g = 0; g < G; ++g)
                    if (top == a.prefix[x][g]) slot = g * select::kDigits + digit;
            }
        }
        const unsigned long long any = __ballot(slot != kNoSlot);
        if (!any) continue;
        const uint32_t lead = (uint32_t)__builtin_ctzll(any);
        const uint32_t first = (uint32_t)__shfl((int)slot, (int)lead, 64);
        const unsigned long long same = __ballot(slot == first);
        if (slot == first) {
            if (lane == lead) atomicAdd(&table[first], (uint32_t)__popcll(same));
        } else if (slot != kNoSlot) {
            atomicAdd(&table[slot], 1u);
        }
    }
    __syncthreads();

    unsigned long long* hist = a.hist + (uint64_t)x * kMaxSelectGroups * select::kDigits;
    for (uint32_t s = tid; s < slots; s += kSelectBlock) {
        const uint32_t c = table[s];
        if (c) atomicAdd(&hist[s], (unsigned long long)c);
    }
}

}  // namespace

hipError_t launch_select_keys(const SelectKeyArgs& a, hipStream_t stream) {
    SelectKeyArgs copy = a;
    void* args[] = {&copy};
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + kSelectBlock - 1) / kSelectBlock);
    return hipLaunchKernel((const void*)ssa_select_keys, dim3(blocks), dim3(kSelectBlock), args, 0, stream);
}

hipError_t launch_select_digits(const SelectArgs& a, hipStream_t stream) {
    SelectArgs copy = a;
    void* args[] = {&copy};
    uint32_t G = 1;
    for (uint32_t x = 0; x < select::kDistances; ++x) G = a.n_groups[x] > G ? a.n_groups[x] : G;
    if (G > kMaxSelectGroups || a.reps_per_block == 0u || a.pass >= select::kPasses) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + a.reps_per_block - 1) / a.reps_per_block);
    return hipLaunchKernel((const void*)ssa_select_digits, dim3(blocks, select::kDistances), dim3(kSelectBlock), args,
                           (size_t)G * select::kDigits * sizeof(uint32_t), stream);
}

}  // namespace ecdna
