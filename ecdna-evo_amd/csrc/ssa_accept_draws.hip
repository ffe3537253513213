// ssa_accept_draws.hip — acceptance over repeated thinnings of the kept samples (gfx950): the pass of
// ecdna_ssa_ctx_accept_draws (thinned acceptance mapping v1, include/ecdna_ssa.h).
//
// The draw index d of thinning mapping v1 gives 64 independent thinnings of one kept sample; the share of them a
// replicate passes estimates its acceptance probability under measurement noise. This pass is ssa_thin and
// ssa_accept_mask run together over a range of draws: per draw the thinned sample is drawn and scored by the code
// ssa_thin draws and scores with (ssa_thinwave.hpp: wave_thin_draw on the slice's thinning stream, wave_thin_record
// over wave_cohort_record, fp contract off), the records stay in registers — lane j holds the record of the j-th
// target of a group's list — and the thresholds are tested on them at once. What is kept is a count.
//
// One wave per replicate, 1, 2 or 4 waves per workgroup, ssa_thin's LDS plan. Per participating slice, in timepoint
// order, the kept row is read once into the full histogram; a group whose m1 reaches a + b is scored once on it, every
// other group once per draw. Lane q keeps row q's 64-bit set of the draws that still pass: a row's verdict over a
// group's targets is a ballot, and a failure clears bit d (a whole-sample group's failure clears the range). The sets
// carry across the slices of a timepoint store, so a draw passes when every participating timepoint passes on it. A draw
// no row can pass any more is not drawn again: its bit is clear in every set whatever the rest would say. A record the
// guards zero (the header's, the size's, the draws') has four zero distances and passes every row, as in the loop of
// ssa_thin and ssa_accept_mask. Lane q stores popcount(set) as byte q of the replicate's Q bytes.
//
// The per-set sums: lane q keeps a running total while the wave's consecutive replicates belong to one global
// parameter set and adds it with one u64 atomic per (wave, set, row) when the set changes and at the end: integer
// adds, exact in any order. No workgroup state and no workgroup barrier.
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

// The rows that the records of a group's targets fail: lane j < count holds the j-th record. Wave-uniform.
__device__ __forceinline__ uint32_t rows_failed(const AcceptDrawsArgs& a, const ecdna_rep_stats_t& rec, uint32_t count,
                                                uint32_t lane) {
    uint32_t failed = 0u;
    for (uint32_t q = 0; q < a.Q; ++q)
        if (__ballot(lane < count && !row_passes(rec, a.thr[q]))) failed |= 1u << q;
    return failed;
}

__global__ void __launch_bounds__(256) ssa_accept_draws(const AcceptDrawsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const DrawsArgs& c = a.s;
    const Grouping& gr = a.g;
    const uint32_t bins = c.bins;
    const ThinLds L = thin_lds(lds, wave, 2u * bins + c.scratch_words, bins);  // (ssa_thin's plan)
    const uint32_t r_begin = blockIdx.x * c.reps_per_block;
    if (r_begin >= c.n) return;
    const uint32_t r_end = min(c.n, r_begin + c.reps_per_block);
    const uint32_t d_end = c.first_draw + c.n_draws;
    const uint64_t range = draws_range(c);

    uint64_t cur_set = ~0ull, total = 0;  // lane q: row q's passes over the wave's replicates of cur_set so far
    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint64_t rid = c.rid0 + (uint64_t)q * c.rid_stride;
        const uint64_t set = rid / c.reps_per_set;
        if (set != cur_set) {
            if (total && cur_set < c.n_sets) atomicAdd(&a.sums[(uint64_t)lane * c.n_sets + cur_set], total);
            cur_set = set;
            total = 0;
        }
        const uint32_t err = draws_error(c, q);                 // rule 1
        uint64_t alive = (lane < a.Q && !err) ? range : 0ull;  // lane q: the draws row q still passes

        for (uint32_t s = 0; s < c.n_slices && !err; ++s) {
            if (!((c.slice_mask >> s) & 1ull)) continue;
            if (__ballot(alive != 0ull) == 0ull) break;  // (nothing is left to decide)
            const KeptSample k = kept_sample(c.headers, c.cells, (uint64_t)s * c.n + q, c.m);
            if (k.guard) continue;  // the guard: all-zero records

            // 1. the one scan: the kept sample's full histogram and its sum of k
            const uint64_t ksum = wave_kept_hist(L.fh, bins, k, lane);

            // 2. each group: the whole kept sample once, or one thinned sample per draw, tested in registers
            for (uint32_t g = gr.slice_group[s]; g < gr.slice_group[s + 1u]; ++g) {
                const uint32_t m1 = gr.group_m[g];
                const uint32_t* list = gr.group_targets + gr.group_offset[g];
                const uint32_t count = gr.group_offset[g + 1u] - gr.group_offset[g];
                const SamplePlan plan = sample_plan(m1, k.cells_all);
                if (plan.bad) continue;  // the guard: all-zero records
                if (plan.whole) {
                    const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, true, false, m1, ksum, 0ull, c.target_cdf,
                                                                   c.target_scalars, list, count, lane);
                    const uint32_t failed = rows_failed(a, rec, count, lane);
                    if (lane < 32u && ((failed >> lane) & 1u)) alive &= ~range;
                    wave_sync_lds();
                    continue;
                }
                for (uint32_t d = c.first_draw; d < d_end; ++d) {
                    if (__ballot((alive >> d) & 1ull) == 0ull) continue;  // no row passes draw d any more
                    uint64_t psum = 0;  // sum of k over the picked positions
                    const bool bad = wave_thin_draw(L, c.table_slots, bins, k, plan, thin::draw_tag(c.slice_tag[s], d),
                                                    c.slice_seed[s], rid, lane, psum);
                    if (!bad) {
                        const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, false, plan.comp, m1, ksum, psum,
                                                                       c.target_cdf, c.target_scalars, list, count, lane);
                        const uint32_t failed = rows_failed(a, rec, count, lane);
                        if (lane < 32u && ((failed >> lane) & 1u)) alive &= ~(1ull << d);
                    }
                    wave_sync_lds();  // wh and the scratch are written again for the next draw, group or slice
                }
            }
        }
        const uint32_t passed = (uint32_t)__popcll(alive);
        if (lane < a.Q) a.passes[(uint64_t)q * a.Q + lane] = (uint8_t)passed;
        total += passed;
    }
    if (total && cur_set < c.n_sets) atomicAdd(&a.sums[(uint64_t)lane * c.n_sets + cur_set], total);
}

}  // namespace

hipError_t launch_accept_draws(const AcceptDrawsArgs& a, hipStream_t stream) {
    AcceptDrawsArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = thin_waves(a.s.bins, a.s.table_slots, &lds);
    // (the kernel indexes its LDS, its tables, the targets and its outputs by these: refuse a block that does not agree
    // with the plan)
    if (lds > kPassLdsMax || !draws_ok(a.s) || !grouping_ok(a.g, a.s.n_slices, a.s.n_targets, a.s.m) || a.Q < 1u ||
        a.Q > kMaxAcceptRows || !a.passes || !a.sums)
        return hipErrorInvalidValue;
    const uint32_t blocks = (a.s.n + a.s.reps_per_block - 1u) / a.s.reps_per_block;
    return hipLaunchKernel((const void*)ssa_accept_draws, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
