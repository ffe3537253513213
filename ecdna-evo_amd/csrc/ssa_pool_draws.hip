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
//   1. The verdict: the 64-bit set of the draws the replicate passes under the row — ssa_accept_draws' lane q's: the
//      same groups, and the draws, records and rule both kernels share (ssa_thinwave.hpp: wave_thin_draw,
//      wave_thin_record, row_passes; fp contract off), for one row, so the set is wave-uniform. The joint verdict over the slices of a timepoint store is
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
#include "ssa_thinwave.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

// Whether any record of a group's targets fails the row: lane j < count holds the j-th record. Wave-uniform.
__device__ __forceinline__ bool row_failed(const PoolDrawsArgs& a, const ecdna_rep_stats_t& rec, uint32_t count,
                                           uint32_t lane) {
    return __ballot(lane < count && !row_passes(rec, a.thr)) != 0ull;
}

__global__ void __launch_bounds__(256) ssa_pool_draws(const PoolDrawsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const DrawsArgs& c = a.s;
    const uint32_t bins = c.bins;
    // (ssa_thin's layout; the accumulator lies behind the table, over the CDF's upper part and past the scratch where
    // that is too small — the CDF is dead while samples are drawn for the pools)
    const ThinLds L = thin_lds(lds, wave, a.wave_words, bins);
    uint32_t* acc = L.tab + c.table_slots;  // [bins] a group's pooled draws
    const uint32_t r_begin = blockIdx.x * c.reps_per_block;
    if (r_begin >= c.n) return;
    const uint32_t r_end = min(c.n, r_begin + c.reps_per_block);
    const uint32_t d_end = c.first_draw + c.n_draws;
    const uint64_t range = draws_range(c);
    const uint64_t set_words = (uint64_t)c.n_sets * bins;

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint64_t rid = c.rid0 + (uint64_t)q * c.rid_stride;
        const uint64_t set = rid / c.reps_per_set;
        if (set >= c.n_sets) continue;
        if (draws_error(c, q)) continue;  // rule 1

        // ---- 1. the verdict: the draws the row still passes (wave-uniform) ----
        uint64_t alive = range;
        uint32_t fh_slice = ~0u;  // the slice whose full histogram fh holds
        for (uint32_t s = 0; s < c.n_slices && alive; ++s) {
            if (!((c.slice_mask >> s) & 1ull)) continue;
            const KeptSample k = kept_sample(c.headers, c.cells, (uint64_t)s * c.n + q, c.m);
            if (k.guard) continue;  // the guard: all-zero records, which pass
            const uint64_t ksum = wave_kept_hist(L.fh, bins, k, lane);
            fh_slice = s;

            const Grouping& gr = a.verdict;
            for (uint32_t g = gr.slice_group[s]; g < gr.slice_group[s + 1u] && alive; ++g) {
                const uint32_t m1 = gr.group_m[g];
                const uint32_t* list = gr.group_targets + gr.group_offset[g];
                const uint32_t count = gr.group_offset[g + 1u] - gr.group_offset[g];
                const SamplePlan plan = sample_plan(m1, k.cells_all);
                if (plan.bad) continue;  // the guard: all-zero records
                if (plan.whole) {
                    const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, true, false, m1, ksum, 0ull, c.target_cdf,
                                                                   c.target_scalars, list, count, lane);
                    if (row_failed(a, rec, count, lane)) alive = 0ull;
                    wave_sync_lds();
                    continue;
                }
                for (uint32_t d = c.first_draw; d < d_end; ++d) {
                    if (!((alive >> d) & 1ull)) continue;  // draw d has failed already
                    uint64_t psum = 0;  // sum of k over the picked positions
                    const bool bad = wave_thin_draw(L, c.table_slots, bins, k, plan, thin::draw_tag(c.slice_tag[s], d),
                                                    c.slice_seed[s], rid, lane, psum);
                    if (!bad) {
                        const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, false, plan.comp, m1, ksum, psum,
                                                                       c.target_cdf, c.target_scalars, list, count, lane);
                        if (row_failed(a, rec, count, lane)) alive &= ~(1ull << d);
                    }
                    wave_sync_lds();  // wh and the scratch are written again for the next draw, group or slice
                }
            }
        }
        if (!alive) continue;
        const uint32_t weight = (uint32_t)__popcll(alive);

        // ---- 2. the pools: every slice, held-out ones included ----
        for (uint32_t s = 0; s < c.n_slices; ++s) {
            const KeptSample k = kept_sample(c.headers, c.cells, (uint64_t)s * c.n + q, c.m);
            if (k.guard) continue;  // the guard adds nothing
            if (fh_slice != s) {
                wave_kept_hist(L.fh, bins, k, lane);
                fh_slice = s;
            }
            if (a.kept) {
                unsigned long long* out = a.kept + ((uint64_t)s * c.n_sets + set) * bins;
                for (uint32_t b = lane; b < bins; b += 64u) {
                    const uint32_t v = L.fh[b];
                    if (v) atomicAdd(&out[b], (unsigned long long)v * weight);
                }
            }
            if (!a.thinned) continue;
            const Grouping& gr = a.pool;
            for (uint32_t g = gr.slice_group[s]; g < gr.slice_group[s + 1u]; ++g) {
                const uint32_t m1 = gr.group_m[g];
                const uint32_t* list = gr.group_targets + gr.group_offset[g];
                const uint32_t count = gr.group_offset[g + 1u] - gr.group_offset[g];
                const SamplePlan plan = sample_plan(m1, k.cells_all);
                if (plan.bad) continue;  // a size the plan refuses adds nothing
                const uint32_t* src = L.fh;
                uint32_t times = weight;
                if (!plan.whole) {
                    for (uint32_t b = lane; b < bins; b += 64u) acc[b] = 0u;
                    for (uint32_t d = c.first_draw; d < d_end; ++d) {
                        if (!((alive >> d) & 1ull)) continue;
                        uint64_t psum = 0;
                        const bool bad = wave_thin_draw(L, c.table_slots, bins, k, plan,
                                                        thin::draw_tag(c.slice_tag[s], d), c.slice_seed[s], rid, lane, psum);
                        // (lane l owns bins l, l + 64, ... of the accumulator throughout)
                        if (!bad)
                            for (uint32_t b = lane; b < bins; b += 64u) acc[b] += L.wh[b];
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
    const uint32_t nw = pool_draws_waves(a.s.bins, a.s.table_slots, &lds);
    // (the kernel indexes its LDS, its tables, the targets and its outputs by these: refuse a block that does not agree
    // with the plan)
    if (lds > kPassLdsMax || !draws_ok(a.s) || a.wave_words != pool_draws_wave_words(a.s.bins, a.s.table_slots) ||
        (a.s.table_slots & 1u) || !grouping_ok(a.verdict, a.s.n_slices, a.s.n_targets, a.s.m) ||
        !grouping_ok(a.pool, a.s.n_slices, a.s.n_targets, a.s.m) || (!a.thinned && !a.kept))
        return hipErrorInvalidValue;
    const uint32_t blocks = (a.s.n + a.s.reps_per_block - 1u) / a.s.reps_per_block;
    return hipLaunchKernel((const void*)ssa_pool_draws, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
