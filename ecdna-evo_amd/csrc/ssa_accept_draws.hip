// ssa_accept_draws.hip — acceptance over repeated thinnings of the kept samples (gfx950): the pass of
// ecdna_ssa_ctx_accept_draws (thinned acceptance mapping v1, include/ecdna_ssa.h).
//
// The draw index d of thinning mapping v1 gives 64 independent thinnings of one kept sample; the share of them a
// replicate passes estimates its acceptance probability under measurement noise. This pass is ssa_thin and
// ssa_accept_mask run together over a range of draws: per draw the thinned sample is drawn and scored exactly as
// ssa_thin does (wave_sample_picks<0> on the slice's thinning stream, wave_cohort_record: wave_cohort_stats' f64
// operations in its lane and scan order, fp contract off), the records stay in registers — lane j holds the record of
// the j-th target of a group's list — and the thresholds are tested on them at once. What is kept is a count.
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
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

// ssa_accept_mask's rule: a tie passes; +inf switches the statistic off, NaN distances included; a NaN distance fails
// every finite threshold.
__device__ __forceinline__ bool passes(double d, double thr) { return thr == __builtin_huge_val() || d <= thr; }

// The rows that the records of a group's targets fail: lane j < count holds the j-th record. Wave-uniform.
__device__ __forceinline__ uint32_t rows_failed(const AcceptDrawsArgs& a, const ecdna_rep_stats_t& rec, uint32_t count,
                                                uint32_t lane) {
    uint32_t failed = 0u;
    for (uint32_t q = 0; q < a.Q; ++q) {
        const bool ok = passes(rec.ks, a.thr[q][0]) && passes(rec.mean_rel, a.thr[q][1]) &&
                        passes(rec.entropy_rel, a.thr[q][2]) && passes(rec.frequency_diff, a.thr[q][3]);
        if (__ballot(lane < count && !ok)) failed |= 1u << q;
    }
    return failed;
}

__global__ void __launch_bounds__(256) ssa_accept_draws(const AcceptDrawsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = a.bins, last = bins - 1u;
    // (ssa_thin's layout: every term is even, so each wave's scratch is 8-byte aligned for the CDF)
    const uint32_t wave_words = 2u * bins + a.scratch_words;
    uint32_t* fh = reinterpret_cast<uint32_t*>(lds) + (size_t)wave * wave_words;  // [bins] the kept sample's histogram
    uint32_t* wh = fh + bins;                                                     // [bins] a thinned sample's
    uint32_t* tab = wh + bins;                                                    // [scratch_words]: the table, or
    double* F = reinterpret_cast<double*>(tab);                                   // [bins] the scored sample's CDF
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);
    const uint32_t d_end = a.first_draw + a.n_draws;
    const uint64_t range = (a.n_draws >= 64u ? ~0ull : (1ull << a.n_draws) - 1ull) << a.first_draw;

    uint64_t cur_set = ~0ull, total = 0;  // lane q: row q's passes over the wave's replicates of cur_set so far
    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const uint64_t rid = a.rid0 + (uint64_t)q * a.rid_stride;
        const uint64_t set = rid / a.reps_per_set;
        if (set != cur_set) {
            if (total && cur_set < a.n_sets) atomicAdd(&a.sums[(uint64_t)lane * a.n_sets + cur_set], total);
            cur_set = set;
            total = 0;
        }
        // rule 1: the one summary, or the summary of every participating phase
        uint32_t err = 0u;
        if (a.err_stride == 0u) {
            err = a.summaries[q].error;
        } else {
            for (uint32_t s = 0; s < a.n_slices; ++s)
                if ((a.slice_mask >> s) & 1ull) err |= a.summaries[(uint64_t)q + s * a.err_stride].error;
        }
        uint64_t alive = (lane < a.Q && !err) ? range : 0ull;  // lane q: the draws row q still passes

        for (uint32_t s = 0; s < a.n_slices && !err; ++s) {
            if (!((a.slice_mask >> s) & 1ull)) continue;
            if (__ballot(alive != 0ull) == 0ull) break;  // (nothing is left to decide)
            const uint64_t at = (uint64_t)s * a.n + q;
            const uint2 h = a.headers[at];
            if (h.x == kKeptGuard && h.y == kKeptGuard) continue;  // the guard: all-zero records
            const uint32_t np = min(h.y, a.m);  // (a row holds m cells)
            const uint64_t cells_all = (uint64_t)h.x + np;
            const uint16_t* row = a.cells + at * a.m;
            const uint32_t k0 = (uint32_t)a.slice_seed[s], k1 = (uint32_t)(a.slice_seed[s] >> 32);

            // 1. the one scan: the kept sample's full histogram and its sum of k, as ssa_thin makes them
            for (uint32_t b = lane; b < bins; b += 64u) fh[b] = 0u;
            wave_sync_lds();
            uint64_t ksum = 0;
            for (uint32_t j = lane; j < np; j += 64u) {
                const uint32_t kk = row[j];
                atomicAdd(&fh[kk < last ? kk : last], 1u);
                ksum += kk;
            }
            if (lane == 0) atomicAdd(&fh[0], h.x);
            wave_sync_lds();
            ksum = wave_sum(ksum);
            const SamplePop pop{(uint64_t)h.x, nullptr, 0u, 0u, row, np};

            // 2. each group: the whole kept sample once, or one thinned sample per draw, tested in registers
            for (uint32_t g = a.slice_group[s]; g < a.slice_group[s + 1u]; ++g) {
                const uint32_t m1 = a.group_m[g];
                const uint32_t* list = a.group_targets + a.group_offset[g];
                const uint32_t count = a.group_offset[g + 1u] - a.group_offset[g];
                const SamplePlan plan = sample_plan(m1, cells_all);
                if (plan.bad) continue;  // the guard: all-zero records
                if (plan.whole) {
                    const ecdna_rep_stats_t rec = wave_cohort_record(fh, F, bins, cells_all, ksum, (uint64_t)np,
                                                                     a.target_cdf, a.target_scalars, list, count, lane);
                    const uint32_t failed = rows_failed(a, rec, count, lane);
                    if (lane < 32u && ((failed >> lane) & 1u)) alive &= ~range;
                    wave_sync_lds();
                    continue;
                }
                for (uint32_t d = a.first_draw; d < d_end; ++d) {
                    if (__ballot((alive >> d) & 1ull) == 0ull) continue;  // no row passes draw d any more
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
    if (total && cur_set < a.n_sets) atomicAdd(&a.sums[(uint64_t)lane * a.n_sets + cur_set], total);
}

}  // namespace

hipError_t launch_accept_draws(const AcceptDrawsArgs& a, hipStream_t stream) {
    AcceptDrawsArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = thin_waves(a.bins, a.table_slots, &lds);
    // (the kernel indexes its LDS, its tables, the targets and its outputs by these: refuse a block that does not agree
    // with the plan)
    if (lds > kPassLdsMax || a.scratch_words != cohort_scratch_words(a.bins, a.table_slots) || a.n_slices < 1u ||
        a.n_slices > kMaxCohortTargets || a.n_targets < 1u || a.n_targets > kMaxCohortTargets || a.n_groups < 1u ||
        a.n_groups > a.n_targets || a.Q < 1u || a.Q > kMaxAcceptRows || a.n_draws < 1u || a.first_draw > thin::kMaxDraw ||
        a.n_draws > thin::kMaxDraw + 1u - a.first_draw || !a.n || !a.reps_per_block || a.bins < 2u || !a.rid_stride ||
        !a.reps_per_set || !a.n_sets || !a.m || !a.slice_mask ||
        (a.n_slices < 64u && (a.slice_mask >> a.n_slices)) || a.slice_group[0] != 0u ||
        a.slice_group[a.n_slices] != a.n_groups || a.group_offset[0] != 0u || a.group_offset[a.n_groups] > a.n_targets ||
        !a.headers || !a.cells || !a.summaries || !a.target_cdf || !a.target_scalars || !a.passes || !a.sums)
        return hipErrorInvalidValue;
    for (uint32_t s = 0; s < a.n_slices; ++s)
        if (a.slice_group[s] > a.slice_group[s + 1u]) return hipErrorInvalidValue;
    for (uint32_t g = 0; g < a.n_groups; ++g)
        if (a.group_offset[g] > a.group_offset[g + 1u] || a.group_m[g] < 1u || a.group_m[g] > a.m)
            return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.group_offset[a.n_groups]; ++j)
        if (a.group_targets[j] >= a.n_targets) return hipErrorInvalidValue;
    const uint32_t blocks = (a.n + a.reps_per_block - 1u) / a.reps_per_block;
    return hipLaunchKernel((const void*)ssa_accept_draws, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
