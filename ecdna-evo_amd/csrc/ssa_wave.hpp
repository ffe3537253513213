// ssa_wave.hpp — the wave-level pieces the end-of-run kernels share (ssa_hist.hip, ssa_subsample.hip, ssa_passage.hip,
// ssa_snapstats.hip, the last three through ssa_sampledraw.hpp too; wave_sum also the development counters of
// ssa_refdraws.hip): wave reductions and the inclusive scan, the wave's LDS ordering
// point, a chunk's parameter-set segments, the bin-counter read, and the one routine for
// the per-replicate ABC statistics, with its sibling for a list of targets (wave_cohort_stats: ssa_cohort.hip and
// ssa_rescore.hip perform the same operations in the same order through it, which is what makes a rescored record the
// launch-time record byte for byte). Plain functions over one 64-lane wave; every lane of the wave calls them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ecdna_ssa.h"

#pragma clang fp contract(off)

namespace ecdna {

// The wave's LDS accesses so far are complete and ordered before its later ones: plain stores (wh[b] = 0) against
// other lanes' later LDS atomics too, which is what the wavefront-scope fence adds to the wait.
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS accesses have completed
    __builtin_amdgcn_wave_barrier();
}

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor((unsigned long long)x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// The lane's inclusive prefix sum over the wave (lanes 0 .. lane); lane 63 holds the wave's total.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if ((int)lane >= o) x += y;
    }
    return x;
}

// Local replicates r .. seg_end - 1 of a chunk share parameter set `set`: their ids rid0 + r * rid_stride lie below
// the set's end (set + 1) * reps_per_set. seg_end <= r_end.
struct SetSegment {
    uint64_t set;
    uint32_t seg_end;
};
__device__ __forceinline__ SetSegment set_segment(uint64_t rid0, uint64_t rid_stride, uint64_t reps_per_set, uint32_t r,
                                                  uint32_t r_end) {
    const uint64_t set = (rid0 + (uint64_t)r * rid_stride) / reps_per_set;
    const uint64_t set_end_rid = (set + 1) * reps_per_set;
    const uint64_t in_set = (set_end_rid - rid0 + rid_stride - 1) / rid_stride;
    return {set, (uint32_t)min((uint64_t)r_end, in_set)};
}

// Bin counter b (copy number b + 1) of replicate q: bags[q][bag_k], u16 (BAG = 1) or u32 (BAG = 2).
template <int BAG>
__device__ __forceinline__ uint32_t bag_counter(const void* bags, uint64_t q, uint32_t bag_k, uint32_t b) {
    const uint64_t o = q * bag_k + b;
    return BAG == 2 ? reinterpret_cast<const uint32_t*>(bags)[o] : (uint32_t)reinterpret_cast<const uint16_t*>(bags)[o];
}

// The ABC statistics of one replicate (or of its sample) from the wave's LDS histogram wh[bins]: mean = ksum / cells,
// entropy, N+ frequency = nplus / cells, the KS distance to target_cdf by a wave prefix scan over the bins, and the
// distances to the target (abc.md:38-55). cells == 0: mean, entropy and frequency 0, ks 1.0 with a target. The
// non-zero bins of wh are added to the workgroup histogram hb on the way. ksum and nplus are wave totals; wh must be
// complete (wave_sync_lds). Lane 0 writes *out.
__device__ __forceinline__ void wave_rep_stats(const uint32_t* wh, unsigned long long* hb, uint32_t bins, uint64_t cells,
                                               uint64_t ksum, uint64_t nplus, uint32_t has_target,
                                               const double* target_cdf, double target_mean, double target_entropy,
                                               double target_freq, uint32_t lane, ecdna_rep_stats_t* out) {
    const double inv = cells ? 1.0 / (double)cells : 0.0;
    double carry = 0.0, ent = 0.0, ks = 0.0;
    for (uint32_t base = 0; base < bins; base += 64u) {
        const uint32_t b = base + lane;
        const uint32_t cnt = b < bins ? wh[b] : 0u;
        if (cnt) atomicAdd(&hb[b], (unsigned long long)cnt);
        const double p = (double)cnt * inv;
        if (cnt) ent -= p * log(p);
        const double scan = wave_inclusive_scan(p, lane);
        if (has_target && b < bins) ks = fmax(ks, fabs(carry + scan - target_cdf[b]));
        carry += __shfl(scan, 63, 64);
    }
    ent = wave_sum(ent);
    ks = wave_max(ks);
    if (lane == 0) {
        ecdna_rep_stats_t st;
        st.cells = cells;
        st.mean = cells ? (double)ksum * inv : 0.0;
        st.entropy = ent;
        st.frequency = cells ? (double)nplus * inv : 0.0;
        st.ks = has_target ? (cells ? ks : 1.0) : 0.0;
        const double dm = fabs(st.mean - target_mean), de = fabs(st.entropy - target_entropy);
        st.mean_rel = has_target ? (target_mean > 0.0 ? dm / target_mean : dm) : 0.0;
        st.entropy_rel = has_target ? (target_entropy > 0.0 ? de / target_entropy : de) : 0.0;
        st.frequency_diff = has_target ? fabs(st.frequency - target_freq) : 0.0;
        *out = st;
    }
}

// The sibling of wave_rep_stats for a list of targets: the statistics of the population whose histogram wh[bins] holds
// against targets list[0 .. count) (list == nullptr: targets 0 .. count - 1), count <= 64, written to
// out[target * out_stride]. Nothing is added to a workgroup histogram. cells, ksum and nplus are wave totals; wh must be
// complete (wave_sync_lds). F[bins] is the wave's scratch for the population's CDF; every lane reads back only the bins
// it wrote (b = lane mod 64). Per target the operations and their order are wave_rep_stats': the lane's
// ks = fmax(ks, |F(b) - F_t(b)|) over its bins ascending, then the wave maximum (max is exact in any order).
//
// wave_cohort_record is the register-level core: lane j < count returns the record of the j-th target of the list (the
// other lanes an unspecified one) and nothing is stored, so a pass that keeps no records (ssa_accept_draws.hip) tests
// the very numbers wave_cohort_stats writes.
__device__ __forceinline__ ecdna_rep_stats_t wave_cohort_record(const uint32_t* wh, double* F, uint32_t bins,
                                                                uint64_t cells, uint64_t ksum, uint64_t nplus,
                                                                const double* target_cdf, const double* target_scalars,
                                                                const uint32_t* list, uint32_t count, uint32_t lane) {
    const double inv = cells ? 1.0 / (double)cells : 0.0;
    double carry = 0.0, ent = 0.0;
    for (uint32_t base = 0; base < bins; base += 64u) {
        const uint32_t b = base + lane;
        const uint32_t cnt = b < bins ? wh[b] : 0u;
        const double p = (double)cnt * inv;
        if (cnt) ent -= p * log(p);
        const double scan = wave_inclusive_scan(p, lane);
        if (b < bins) F[b] = carry + scan;
        carry += __shfl(scan, 63, 64);
    }
    ent = wave_sum(ent);
    double my_ks = 0.0;  // lane j: the KS distance to the j-th target of the list
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t t = list ? list[j] : j;
        const double* tc = target_cdf + (uint64_t)t * bins;
        double ks = 0.0;
        for (uint32_t b = lane; b < bins; b += 64u) ks = fmax(ks, fabs(F[b] - tc[b]));
        ks = wave_max(ks);
        if (lane == j) my_ks = ks;
    }
    ecdna_rep_stats_t st{};
    if (lane < count) {
        const uint32_t t = list ? list[lane] : lane;
        const double target_mean = target_scalars[3u * t], target_entropy = target_scalars[3u * t + 1u],
                     target_freq = target_scalars[3u * t + 2u];
        st.cells = cells;
        st.mean = cells ? (double)ksum * inv : 0.0;
        st.entropy = ent;
        st.frequency = cells ? (double)nplus * inv : 0.0;
        st.ks = cells ? my_ks : 1.0;
        const double dm = fabs(st.mean - target_mean), de = fabs(st.entropy - target_entropy);
        st.mean_rel = target_mean > 0.0 ? dm / target_mean : dm;
        st.entropy_rel = target_entropy > 0.0 ? de / target_entropy : de;
        st.frequency_diff = fabs(st.frequency - target_freq);
    }
    return st;
}

__device__ __forceinline__ void wave_cohort_stats(const uint32_t* wh, double* F, uint32_t bins, uint64_t cells,
                                                  uint64_t ksum, uint64_t nplus, const double* target_cdf,
                                                  const double* target_scalars, const uint32_t* list, uint32_t count,
                                                  uint32_t lane, ecdna_rep_stats_t* out, uint64_t out_stride) {
    const ecdna_rep_stats_t st =
        wave_cohort_record(wh, F, bins, cells, ksum, nplus, target_cdf, target_scalars, list, count, lane);
    if (lane < count) out[(uint64_t)(list ? list[lane] : lane) * out_stride] = st;
}

}  // namespace ecdna
