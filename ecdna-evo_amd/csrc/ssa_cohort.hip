// ssa_cohort.hip — one sweep scored against a cohort of targets (gfx950): the end-of-run pass of ecdna_ssa_cohort_t
// (cohort mapping v1, include/ecdna_ssa.h).
//
// A cohort is several patients, or several biopsies of one tumour, each with its own copy-number histogram and its own
// number of measured cells. The simulations do not depend on the target, so this pass, after ssa_hist and ssa_subsample
// on the same stream, scores every replicate's final state against all P targets where that state lies: record
// stats[p][i] is byte for byte what ssa_hist<true, BAG> writes for the run with target p, and sample_stats[p][i] what
// ssa_subsample writes for it with target p and p's sample size. Both hold because the statistics are IEEE f64
// operations over integers in a fixed lane and scan order (fp contract off), and wave_cohort_stats (ssa_wave.hpp)
// performs the operations of wave_rep_stats in its order; the draws are wave_sample_picks' on the end-of-run stream.
//
// One wave per replicate, as ssa_subsample. The final state is scanned once, into the full histogram fh, which stays in
// LDS: the target-independent part of the statistics (probabilities, their prefix scan, entropy) is computed once per
// histogram, the population's CDF is kept in LDS (f64 per bin) and each target takes its KS distance against it. The
// targets are grouped by distinct sample size (ssa_cohort.hpp): a group's sample is drawn once — into wh, which starts
// from zero or, for a complement, from a copy of fh — and scored against every target of the group. The CDF shares its
// LDS with the table of drawn positions: one is dead while the other lives. The cohort keeps no pooled histogram, so
// there is no workgroup state and no workgroup barrier. Lane j of the wave finishes the record of the j-th target of a
// list (P <= 64) and writes it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

constexpr uint32_t kCohortBlock = 256;

// BAG as in ssa_hist: 0 = rows only; 1 / 2 = u16 / u32 bin counters bags[q][bag_k] for copy numbers 1..bag_k plus
// the large-k cells at the head of the row.
template <int BAG>
__global__ void __launch_bounds__(kCohortBlock) ssa_cohort(const CohortArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const ChunkIds& ids = a.ids;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = ids.bins;
    // (every term is even, so each wave's scratch is 8-byte aligned for the CDF)
    const uint32_t wave_words = 2u * bins + a.state.bag_k + a.scratch_words;
    uint32_t* fh = reinterpret_cast<uint32_t*>(lds) + (size_t)wave * wave_words;  // [bins] the full histogram
    uint32_t* wh = fh + bins;                                                     // [bins] a sample's histogram
    uint32_t* pre = wh + bins;                                                    // [bag_k]
    uint32_t* tab = pre + a.state.bag_k;                                          // [scratch_words]: the table, or
    double* F = reinterpret_cast<double*>(tab);                                   // [bins] the scored population's CDF
    const uint32_t r_begin = blockIdx.x * ids.reps_per_block;
    if (r_begin >= ids.n) return;
    const uint32_t r_end = min(ids.n, r_begin + ids.reps_per_block);
    const uint32_t last = bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const ecdna_rep_summary_t* s = a.state.summaries + q;
        const uint64_t nm = s->nminus;
        const uint32_t np = (uint32_t)s->nplus;
        const uint64_t cells_all = nm + (uint64_t)np;
        const uint64_t rid = ids.rid0 + (uint64_t)q * ids.rid_stride;

        // 1. the one scan: the full histogram, the prefix sums for the position -> k lookup, the sum of k (the plan of a
        // whole-population sample makes wave_load_final_state build all three)
        SamplePlan full{true, false, (uint32_t)cells_all, 0u, false, true};
        uint64_t ksum = 0;
        const SamplePop pop = wave_load_final_state<BAG>(a.state, q, nm, np, bins, full, fh, pre, ksum, lane);
        wave_sync_lds();
        ksum = wave_sum(ksum);

        // 2. the whole population against all P targets
        wave_cohort_stats(fh, F, bins, cells_all, ksum, np, a.target_cdf, a.target_scalars, nullptr, a.n_targets, lane,
                          a.stats + q, a.out_stride);
        wave_sync_lds();  // the CDF has been read: its words are the table's again

        // 3. each distinct sample size: one sample, scored against the group's targets
        for (uint32_t g = 0; g < a.n_groups; ++g) {
            const uint32_t m = a.group_m[g];
            const uint32_t* list = a.group_targets + a.group_offset[g];
            const uint32_t count = a.group_offset[g + 1u] - a.group_offset[g];
            const SamplePlan plan = sample_plan(m, cells_all);
            // (counters that hold more cells than the summary: wave_load_final_state's guard for a drawn sample)
            bool bad = plan.bad || (BAG != 0 && !plan.whole && pop.small > np);
            uint64_t psum = 0;  // sum of k over the picked positions
            if (!plan.whole && !bad) {
                // the picks are counted into zeros, or taken out of a copy of the full histogram (complement)
                for (uint32_t b = lane; b < bins; b += 64u) wh[b] = plan.comp ? fh[b] : 0u;
                wave_sync_lds();
                bad = wave_sample_picks<BAG>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                             sample_stream_tag(0u), rid, k0, k1, lane, psum);
                wave_sync_lds();
            }
            psum = wave_sum(psum);
            if (bad) {  // the guard: all-zero statistics, as wave_sample_stats
                if (lane < count) a.sample_stats[q + (uint64_t)list[lane] * a.out_stride] = ecdna_rep_stats_t{};
            } else {
                const uint32_t* h = plan.whole ? fh : wh;
                const uint64_t cells = plan.whole ? cells_all : (uint64_t)m;
                const uint64_t ks_sum = plan.whole ? ksum : (plan.comp ? ksum - psum : psum);
                const uint64_t nplus_s = plan.whole ? (uint64_t)np : cells - (uint64_t)wh[0];
                wave_cohort_stats(h, F, bins, cells, ks_sum, nplus_s, a.target_cdf, a.target_scalars, list, count, lane,
                                  a.sample_stats + q, a.out_stride);
            }
            wave_sync_lds();  // wh and the scratch are written again for the next group or replicate
        }
    }
}

}  // namespace

hipError_t launch_cohort(const CohortArgs& a, uint32_t blocks, hipStream_t stream) {
    CohortArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = cohort_waves(a.ids.bins, a.state.bag_k, a.table_slots, &lds);
    // (the kernel indexes its LDS and its groups by these: refuse a block that does not agree with the plan)
    if (lds > kPassLdsMax || a.scratch_words != cohort_scratch_words(a.ids.bins, a.table_slots) ||
        a.n_targets < 1u || a.n_targets > kMaxCohortTargets || a.n_groups > a.n_targets ||
        (a.n_groups && (!a.sample_stats || a.group_offset[a.n_groups] > a.n_targets)))
        return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_cohort<0>, (const void*)ssa_cohort<1>,
                                         (const void*)ssa_cohort<2>};
    return hipLaunchKernel(table[bag_index(a.state)], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
