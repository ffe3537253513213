// ssa_pool_draws.hip — the accepted thinnings of the kept samples, pooled (gfx950): the pass of
// ecdna_ssa_ctx_pool_draws (thinned pooling mapping v1, include/ecdna_ssa.h).
//
// ecdna_ssa_ctx_accept_draws counts on how many thinning draws a replicate is accepted. This pass pools what was
// accepted: per global parameter set, the histograms of the thinned samples on the draws that pass one threshold row
// (the posterior predictive of the measurement itself), and the whole kept samples weighted by the number of passing
// draws. Nothing but integers is pooled: no f64 and no dependence on order.
//
// One wave per replicate, 1, 2 or 4 waves per workgroup, ssa_thin's LDS plan plus one [bins] u32 accumulator per wave,
// which lies behind the table of drawn positions where the scratch has room (ssa_launch.h pool_draws_wave_words).
// A replicate goes through two phases.
//   1. The verdict: the 64-bit set of the draws the replicate passes under the row, computed as ssa_accept_draws
//      computes lane q's — the same groups, draws, records (wave_sample_picks<0>, wave_cohort_record: fp contract off)
//      and rule, for one row, so the set is wave-uniform. The joint verdict over the slices of a timepoint store is
//      known only after the last participating slice: hence a second phase. An empty set ends the replicate here.
//   2. The pools, over every slice of the store, held-out ones included. The slice's full histogram fh is rebuilt (the
//      keep store's one slice still holds it from the verdict) and goes into the kept pool popcount(set) times. Per
//      group of the pooling grouping the thinned sample of every passing draw is drawn again into wh and added to the
//      wave's accumulator, at most 64 x 4096 per bin; a group scored whole adds popcount(set) x fh. The accumulator is
//      flushed once per (replicate, group) into the rows of the group's targets, one u64 atomic per non-zero bin.
// A guard header, a size the plan refuses and the 2^16-draw guard add nothing. No workgroup state and no workgroup
// barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_thin.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

// ssa_accept_mask's rule (ssa_accept_draws.hip): a tie passes; +inf switches the statistic off, NaN distances
// included; a NaN distance fails every finite threshold.
__device__ __forceinline__ bool passes(double d, double thr) { return thr == __builtin_huge_val() || d <= thr; }

// Whether any record of a group's targets fails the row: lane j < count holds the j-th record. Wave-uniform.
__device__ __forceinline__ bool row_failed(const PoolDrawsArgs& a, const ecdna_rep_stats_t& rec, uint32_t count,
                                           uint32_t lane) {
    const bool ok = passes(rec.ks, a.thr[0]) && passes(rec.mean_rel, a.thr[1]) && passes(rec.entropy_rel, a.thr[2]) &&
                    passes(rec.frequency_diff, a.thr[3]);
    return __ballot(lane < count && !ok) != 0ull;
}

// The kept sample's full histogram (N- cells in bin 0, true copy numbers clipped at `last`) into fh, as ssa_thin makes
// it; returns the wave's sum of k.
__device__ __forceinline__ uint64_t full_hist(uint32_t* fh, uint32_t bins, uint32_t last, const uint16_t* row,
                                              uint32_t np, uint32_t a_cells, uint32_t lane) {
    for (uint32_t b = lane; b < bins; b += 64u) fh[b] = 0u;
    wave_sync_lds();
    uint64_t ksum = 0;
    for (uint32_t j = lane; j < np; j += 64u) {
        const uint32_t kk = row[j];
        atomicAdd(&fh[kk < last ? kk : last], 1u);
        ksum += kk;
    }
    if (lane == 0) atomicAdd(&fh[0], a_cells);
    wave_sync_lds();
    return wave_sum(ksum);
}

__global__ void __launch_bounds__(256) ssa_pool_draws(const PoolDrawsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = a.bins, last = bins - 1u;
    // (ssa_thin's layout; the accumulator lies behind the table, over the CDF's upper part and past the scratch where
    // that is too small — the CDF is dead while samples are drawn for the pools. Every term of wave_words is even, so
    // each wave's scratch is 8-byte aligned for the CDF.)
    const uint32_t wave_words = a.wave_words;
    uint32_t* fh = reinterpret_cast<uint32_t*>(lds) + (size_t)wave * wave_words;  // [bins] the kept sample's histogram
    uint32_t* wh = fh + bins;                                                     // [bins] a thinned sample's
    uint32_t* tab = wh + bins;                                                    // [scratch_words]: the table, or
    double* F = reinterpret_cast<double*>(tab);                                   // [bins] the scored sample's CDF
    uint32_t* acc = tab + a.table_slots;                                          // [bins] a group's pooled draws
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);
    const uint32_t d_end = a.first_draw + a.n_draws;
    const uint64_t range = (a.n_draws >= 64u ? ~0ull : (1ull << a.n_draws) - 1ull) << a.first_draw;
    const uint64_t set_words = (uint64_t)a.n_sets * bins;

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint64_t rid = a.rid0 + (uint64_t)q * a.rid_stride;
        const uint64_t set = rid / a.reps_per_set;
        if (set >= a.n_sets) continue;
        // rule 1: the one summary, or the summary of every participating phase
        uint32_t err = 0u;
        if (a.err_stride == 0u) {
            err = a.summaries[q].error;
        } else {
            for (uint32_t s = 0; s < a.n_slices; ++s)
                if ((a.slice_mask >> s) & 1ull) err |= a.summaries[(uint64_t)q + s * a.err_stride].error;
        }
        if (err) continue;

        // ---- 1. the verdict: the draws the row still passes (wave-uniform) ----
        uint64_t alive = range;
        uint32_t fh_slice = ~0u;  // the slice whose full histogram fh holds
        for (uint32_t s = 0; s < a.n_slices && alive; ++s) {
            if (!((a.slice_mask >> s) & 1ull)) continue;
            const uint64_t at = (uint64_t)s * a.n + q;
            const uint2 h = a.headers[at];
            if (h.x == kKeptGuard && h.y == kKeptGuard) continue;  // the guard: all-zero records, which pass
            const uint32_t np = min(h.y, a.m);                    // (a row holds m cells)
            const uint64_t cells_all = (uint64_t)h.x + np;
            const uint16_t* row = a.cells + at * a.m;
            const uint32_t k0 = (uint32_t)a.slice_seed[s], k1 = (uint32_t)(a.slice_seed[s] >> 32);
            const uint64_t ksum = full_hist(fh, bins, last, row, np, h.x, lane);
            fh_slice = s;
            const SamplePop pop{(uint64_t)h.x, nullptr, 0u, 0u, row, np};

            for (uint32_t g = a.v_slice_group[s]; g < a.v_slice_group[s + 1u] && alive; ++g) {
                const uint32_t m1 = a.v_group_m[g];
                const uint32_t* list = a.v_group_targets + a.v_group_offset[g];
                const uint32_t count = a.v_group_offset[g + 1u] - a.v_group_offset[g];
                const SamplePlan plan = sample_plan(m1, cells_all);
                if (plan.bad) continue;  // the guard: all-zero records
                if (plan.whole) {
                    const ecdna_rep_stats_t rec = wave_cohort_record(fh, F, bins, cells_all, ksum, (uint64_t)np,
                                                                     a.target_cdf, a.target_scalars, list, count, lane);
                    if (row_failed(a, rec, count, lane)) alive = 0ull;
                    wave_sync_lds();
                    continue;
                }
                for (uint32_t d = a.first_draw; d < d_end; ++d) {
                    if (!((alive >> d) & 1ull)) continue;  // draw d has failed already
                    // the picks are counted into zeros, or taken out of a copy of the full histogram (complement)
                    for (uint32_t b = lane; b < bins; b += 64u) wh[b] = plan.comp ? fh[b] : 0u;
                    wave_sync_lds();
                    uint64_t psum = 0;  // sum of k over the picked positions
                    const bool bad = wave_sample_picks<0>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                                          a.slice_tag[s] | (d << 10), rid, k0, k1, lane, psum);
                    wave_sync_lds();
                    psum = wave_sum(psum);
                    if (!bad) {
                        const uint64_t ks_sum = plan.comp ? ksum - psum : psum;
                        const uint64_t nplus_s = (uint64_t)m1 - (uint64_t)wh[0];
                        const ecdna_rep_stats_t rec = wave_cohort_record(wh, F, bins, (uint64_t)m1, ks_sum, nplus_s,
                                                                         a.target_cdf, a.target_scalars, list, count, lane);
                        if (row_failed(a, rec, count, lane)) alive &= ~(1ull << d);
                    }
                    wave_sync_lds();  // wh and the scratch are written again for the next draw, group or slice
                }
            }
        }
        if (!alive) continue;
        const uint32_t weight = (uint32_t)__popcll(alive);

        // ---- 2. the pools: every slice, held-out ones included ----
        for (uint32_t s = 0; s < a.n_slices; ++s) {
            const uint64_t at = (uint64_t)s * a.n + q;
            const uint2 h = a.headers[at];
            if (h.x == kKeptGuard && h.y == kKeptGuard) continue;  // the guard adds nothing
            const uint32_t np = min(h.y, a.m);
            const uint64_t cells_all = (uint64_t)h.x + np;
            const uint16_t* row = a.cells + at * a.m;
            const uint32_t k0 = (uint32_t)a.slice_seed[s], k1 = (uint32_t)(a.slice_seed[s] >> 32);
            if (fh_slice != s) {
                full_hist(fh, bins, last, row, np, h.x, lane);
                fh_slice = s;
            }
            if (a.kept) {
                unsigned long long* out = a.kept + ((uint64_t)s * a.n_sets + set) * bins;
                for (uint32_t b = lane; b < bins; b += 64u) {
                    const uint32_t v = fh[b];
                    if (v) atomicAdd(&out[b], (unsigned long long)v * weight);
                }
            }
            if (!a.thinned) continue;
            const SamplePop pop{(uint64_t)h.x, nullptr, 0u, 0u, row, np};
            for (uint32_t g = a.p_slice_group[s]; g < a.p_slice_group[s + 1u]; ++g) {
                const uint32_t m1 = a.p_group_m[g];
                const uint32_t* list = a.p_group_targets + a.p_group_offset[g];
                const uint32_t count = a.p_group_offset[g + 1u] - a.p_group_offset[g];
                const SamplePlan plan = sample_plan(m1, cells_all);
                if (plan.bad) continue;  // a size the plan refuses adds nothing
                const uint32_t* src = fh;
                uint32_t times = weight;
                if (!plan.whole) {
                    for (uint32_t b = lane; b < bins; b += 64u) acc[b] = 0u;
                    for (uint32_t d = a.first_draw; d < d_end; ++d) {
                        if (!((alive >> d) & 1ull)) continue;
                        for (uint32_t b = lane; b < bins; b += 64u) wh[b] = plan.comp ? fh[b] : 0u;
                        wave_sync_lds();
                        uint64_t psum = 0;
                        const bool bad = wave_sample_picks<0>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                                              a.slice_tag[s] | (d << 10), rid, k0, k1, lane, psum);
                        wave_sync_lds();
                        // (lane l owns bins l, l + 64, ... of the accumulator throughout)
                        if (!bad)
                            for (uint32_t b = lane; b < bins; b += 64u) acc[b] += wh[b];
                        wave_sync_lds();  // wh and the table are written again for the next draw
                    }
                    src = acc;
                    times = 1u;
                }
                for (uint32_t b = lane; b < bins; b += 64u) {
                    const unsigned long long v = (unsigned long long)src[b] * times;
                    if (!v) continue;
                    for (uint32_t j = 0; j < count; ++j)
                        atomicAdd(&a.thinned[(uint64_t)list[j] * set_words + set * bins + b], v);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_pool_draws(const PoolDrawsArgs& a, hipStream_t stream) {
    PoolDrawsArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = pool_draws_waves(a.bins, a.table_slots, &lds);
    // (the kernel indexes its LDS, its tables, the targets and its outputs by these: refuse a block that does not agree
    // with the plan)
    if (lds > kPassLdsMax || a.scratch_words != cohort_scratch_words(a.bins, a.table_slots) ||
        a.wave_words != pool_draws_wave_words(a.bins, a.table_slots) || (a.table_slots & 1u) || a.n_slices < 1u ||
        a.n_slices > kMaxCohortTargets || a.n_targets < 1u || a.n_targets > kMaxCohortTargets || a.v_groups < 1u ||
        a.v_groups > a.n_targets || a.p_groups < 1u || a.p_groups > a.n_targets || a.n_draws < 1u ||
        a.first_draw > thin::kMaxDraw || a.n_draws > thin::kMaxDraw + 1u - a.first_draw || !a.n || !a.reps_per_block ||
        a.bins < 2u || !a.rid_stride || !a.reps_per_set || !a.n_sets || !a.m || !a.slice_mask ||
        (a.n_slices < 64u && (a.slice_mask >> a.n_slices)) || a.v_slice_group[0] != 0u ||
        a.v_slice_group[a.n_slices] != a.v_groups || a.v_group_offset[0] != 0u ||
        a.v_group_offset[a.v_groups] > a.n_targets || a.p_slice_group[0] != 0u ||
        a.p_slice_group[a.n_slices] != a.p_groups || a.p_group_offset[0] != 0u ||
        a.p_group_offset[a.p_groups] > a.n_targets || !a.headers || !a.cells || !a.summaries || !a.target_cdf ||
        !a.target_scalars || (!a.thinned && !a.kept))
        return hipErrorInvalidValue;
    for (uint32_t s = 0; s < a.n_slices; ++s)
        if (a.v_slice_group[s] > a.v_slice_group[s + 1u] || a.p_slice_group[s] > a.p_slice_group[s + 1u])
            return hipErrorInvalidValue;
    for (uint32_t g = 0; g < a.v_groups; ++g)
        if (a.v_group_offset[g] > a.v_group_offset[g + 1u] || a.v_group_m[g] < 1u || a.v_group_m[g] > a.m)
            return hipErrorInvalidValue;
    for (uint32_t g = 0; g < a.p_groups; ++g)
        if (a.p_group_offset[g] > a.p_group_offset[g + 1u] || a.p_group_m[g] < 1u || a.p_group_m[g] > a.m)
            return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.v_group_offset[a.v_groups]; ++j)
        if (a.v_group_targets[j] >= a.n_targets) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.p_group_offset[a.p_groups]; ++j)
        if (a.p_group_targets[j] >= a.n_targets) return hipErrorInvalidValue;
    const uint32_t blocks = (a.n + a.reps_per_block - 1u) / a.reps_per_block;
    return hipLaunchKernel((const void*)ssa_pool_draws, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
