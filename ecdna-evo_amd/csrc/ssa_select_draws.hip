// ssa_select_draws.hip — the keys of the select over thinning draws (gfx950): the pass of ecdna_ssa_ctx_select_draws
// and ecdna_ssa_ctx_select_draws_digits (thinned select mapping v1, include/ecdna_ssa.h).
//
// In ABC with measurement noise the population a quantile cuts is the pseudo-datasets, the pairs (replicate, thinning
// draw). This pass is ssa_accept_draws with the threshold test taken out and a key kept in its place: per draw the
// thinned sample is drawn and scored by the code ssa_thin draws and scores with (ssa_thinwave.hpp: wave_thin_draw on
// the slice's thinning stream, wave_thin_record over wave_cohort_record, fp contract off), the records stay in
// registers — lane j holds the record of the j-th target of a group's list — and what is kept of them is, per
// distance, the maximum of their keys (select::key_of, the function ssa_select_keys calls on stored records). The
// digit passes over the keys are ssa_select_digits', unchanged.
//
// One wave per replicate, 1, 2 or 4 waves per workgroup, ssa_thin's LDS plan. Lane d keeps the four running keys of
// draw d, so the wave's 64 lanes hold the 64 draws. Per participating slice, in timepoint order, the kept row is read
// once into the full histogram; a group whose m1 reaches a + b is scored once on it and every lane of the range folds
// its keys in, every other group is drawn and scored once per draw and lane d folds that draw's keys in. A record the
// guards zero (the header's, the size's, the draws') has four zero distances: it contributes key(0.0). There is no
// early exit: every draw of every participating group is drawn. At the end lane d of the range stores its keys at
// entry i * n_draws + (d - first_draw) of each distance's array, so a wave writes four contiguous runs; a replicate
// with an error stores select::kExcluded there. No workgroup state and no workgroup barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_select.hpp"
#include "ssa_thin.hpp"
#include "ssa_thinwave.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

// A lane's four running keys, one per distance in the order of ecdna_accept_threshold_t.
struct Keys {
    uint64_t k[select::kDistances];
};
__device__ __forceinline__ void fold(Keys& into, const Keys& x) {
#pragma unroll
    for (uint32_t j = 0; j < select::kDistances; ++j) into.k[j] = x.k[j] > into.k[j] ? x.k[j] : into.k[j];
}

// Per distance the maximum key over the records of a group's targets: lane j < count holds the j-th record.
// Wave-uniform. (0 is below every key of a number, so the lanes at or above count do not take part.)
__device__ __forceinline__ Keys group_keys(const ecdna_rep_stats_t& rec, uint32_t count, uint32_t lane) {
    const bool mine = lane < count;
    Keys x;
    x.k[0] = wave_max_u64(mine ? select::key_of(rec.ks) : 0ull);
    x.k[1] = wave_max_u64(mine ? select::key_of(rec.mean_rel) : 0ull);
    x.k[2] = wave_max_u64(mine ? select::key_of(rec.entropy_rel) : 0ull);
    x.k[3] = wave_max_u64(mine ? select::key_of(rec.frequency_diff) : 0ull);
    return x;
}

__global__ void __launch_bounds__(256) ssa_select_draws_keys(const SelectDrawsArgs a) {
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
    const bool in_range = (draws_range(c) >> lane) & 1ull;  // lane d: draw d is one of the call's
    const uint64_t total = (uint64_t)c.n * c.n_draws;       // the keys of one distance
    const uint64_t zero_key = select::key_of(0.0);
    const Keys zero{{zero_key, zero_key, zero_key, zero_key}};  // a guarded record's: four zero distances

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint64_t rid = c.rid0 + (uint64_t)q * c.rid_stride;
        const uint32_t err = draws_error(c, q);  // rule 1
        Keys mine{{0ull, 0ull, 0ull, 0ull}};     // lane d: the maximum so far over the records of draw d

        for (uint32_t s = 0; s < c.n_slices && !err; ++s) {
            if (!((c.slice_mask >> s) & 1ull)) continue;
            const KeptSample k = kept_sample(c.headers, c.cells, (uint64_t)s * c.n + q, c.m);
            if (k.guard) {  // the guard: all-zero records, on every draw
                fold(mine, zero);
                continue;
            }

            // 1. the one scan: the kept sample's full histogram and its sum of k
            const uint64_t ksum = wave_kept_hist(L.fh, bins, k, lane);

            // 2. each group: the whole kept sample once, or one thinned sample per draw, its keys taken in registers
            for (uint32_t g = gr.slice_group[s]; g < gr.slice_group[s + 1u]; ++g) {
                const uint32_t m1 = gr.group_m[g];
                const uint32_t* list = gr.group_targets + gr.group_offset[g];
                const uint32_t count = gr.group_offset[g + 1u] - gr.group_offset[g];
                const SamplePlan plan = sample_plan(m1, k.cells_all);
                if (plan.bad) {  // the guard: all-zero records
                    fold(mine, zero);
                    continue;
                }
                if (plan.whole) {
                    const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, true, false, m1, ksum, 0ull, c.target_cdf,
                                                                   c.target_scalars, list, count, lane);
                    fold(mine, group_keys(rec, count, lane));  // one record, counted on every draw
                    wave_sync_lds();
                    continue;
                }
                for (uint32_t d = c.first_draw; d < d_end; ++d) {
                    uint64_t psum = 0;  // sum of k over the picked positions
                    const bool bad = wave_thin_draw(L, c.table_slots, bins, k, plan, thin::draw_tag(c.slice_tag[s], d),
                                                    c.slice_seed[s], rid, lane, psum);
                    Keys x = zero;  // (the guard: an all-zero record)
                    if (!bad) {
                        const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, false, plan.comp, m1, ksum, psum,
                                                                       c.target_cdf, c.target_scalars, list, count, lane);
                        x = group_keys(rec, count, lane);
                    }
                    if (lane == d) fold(mine, x);
                    wave_sync_lds();  // wh and the scratch are written again for the next draw, group or slice
                }
            }
        }
        if (in_range) {
            const uint64_t at = (uint64_t)q * c.n_draws + (lane - c.first_draw);
#pragma unroll
            for (uint32_t j = 0; j < select::kDistances; ++j)
                a.keys[(uint64_t)j * total + at] = err ? select::kExcluded : mine.k[j];
        }
    }
}

}  // namespace

hipError_t launch_select_draws_keys(const SelectDrawsArgs& a, hipStream_t stream) {
    SelectDrawsArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = thin_waves(a.s.bins, a.s.table_slots, &lds);
    // (the kernel indexes its LDS, its tables, the targets and its keys by these: refuse a block that does not agree
    // with the plan)
    if (lds > kPassLdsMax || !draws_ok(a.s) || !grouping_ok(a.g, a.s.n_slices, a.s.n_targets, a.s.m) || !a.keys ||
        (uint64_t)a.s.n * a.s.n_draws >= (1ull << 32))
        return hipErrorInvalidValue;
    const uint32_t blocks = (a.s.n + a.s.reps_per_block - 1u) / a.s.reps_per_block;
    return hipLaunchKernel((const void*)ssa_select_draws_keys, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
