// ssa_thin.hip — the kept samples rescored at each target's own number of measured cells (gfx950): the pass of
// ecdna_ssa_ctx_rescore_sized and _rescore_timepoints_sized (thinning mapping v1, include/ecdna_ssa.h).
//
// A kept sample is {a, b} and the b true copy numbers, ascending. It is a uniform sample of its population, so a uniform
// sample of m1 of its cells has the law of having measured m1 cells of that population: a target with m1 measured cells
// is scored on that thinned sample. The kept sample is the population "a N- cells, then the row" — the shape of a
// snapshot's population, rows only — and the thinned sample is subsample mapping v1's over it (wave_sample_picks<0>,
// ssa_sampledraw.hpp) under the key the kept sample was drawn under, on the kept sample's own stream with the thinning
// flag and the target's draw index set (ssa_thin.hpp stream_tag). A target whose m1 reaches a + b is scored on the
// whole kept sample, and its record is ssa_rescore's byte for byte: the histogram and the sums are integers, and the
// f64 operations on them are wave_cohort_stats' (ssa_wave.hpp) in its lane and scan order (fp contract off).
//
// One wave per replicate, as ssa_rescore. The scan, the thinned draw and the record of a group are ssa_thinwave.hpp's,
// shared with ssa_accept_draws and ssa_pool_draws; this kernel stores the records. The row is read once
// into the full histogram fh, which stays in LDS. The targets are grouped by (m1, draw index)
// (ssa_thin.hpp): a group's sample is drawn once — into wh, which starts from zero or, for a complement, from a copy of
// fh — and scored against every target of the group. Whether a group takes the whole kept sample depends on the
// replicate's a + b: the branch is wave-uniform. The CDF shares its LDS with the table of drawn positions, as in
// ssa_cohort: one is dead while the other lives. No workgroup state and no workgroup barrier. Lane j of the wave
// finishes the record of the j-th target of a group's list and writes it.
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

// the thinning stream is the sampling passes' with bit 29 set: the host's tag function and the device's agree
static_assert(thin::stream_tag(0u, 0u) == (sample_stream_tag(0u) | thin::kThinFlag), "thinning tag");
static_assert(thin::stream_tag(64u, 0u) == (sample_stream_tag(64u) | thin::kThinFlag), "thinning tag");
static_assert((thin::stream_tag(64u, thin::kMaxDraw) & (kSubMaxBlocks - 1u)) == 0u, "the block index's bits are free");

namespace {

__global__ void __launch_bounds__(256) ssa_thin(const ThinArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t bins = a.bins;
    const ThinLds L = thin_lds(lds, wave, 2u * bins + a.scratch_words, bins);
    const uint32_t r_begin = blockIdx.x * a.reps_per_block;
    if (r_begin >= a.n) return;
    const uint32_t r_end = min(a.n, r_begin + a.reps_per_block);

    for (uint32_t q = r_begin + wave; q < r_end; q += nw) {
        const KeptSample k = kept_sample(a.headers, a.cells, q, a.m);
        if (k.guard) {  // the guard: all-zero statistics, as ssa_rescore
            if (lane < a.n_targets) a.out[q + (uint64_t)lane * a.n] = ecdna_rep_stats_t{};
            continue;
        }
        const uint64_t rid = a.rid0 + (uint64_t)q * a.rid_stride;

        // 1. the one scan: the kept sample's full histogram and its sum of k, as ssa_rescore makes them
        const uint64_t ksum = wave_kept_hist(L.fh, bins, k, lane);

        // 2. each (m1, draw index): the whole kept sample, or one thinned sample, scored against the group's targets
        for (uint32_t g = 0; g < a.n_groups; ++g) {
            const uint32_t m1 = a.group_m[g];
            const uint32_t* list = a.group_targets + a.group_offset[g];
            const uint32_t count = a.group_offset[g + 1u] - a.group_offset[g];
            const SamplePlan plan = sample_plan(m1, k.cells_all);
            bool bad = plan.bad;
            uint64_t psum = 0;  // sum of k over the picked positions
            if (!plan.whole && !bad)
                bad = wave_thin_draw(L, a.table_slots, bins, k, plan, a.group_tag[g], a.seed, rid, lane, psum);
            if (bad) {  // the guard: all-zero statistics, as wave_sample_stats
                if (lane < count) a.out[q + (uint64_t)list[lane] * a.n] = ecdna_rep_stats_t{};
            } else {
                const ecdna_rep_stats_t rec = wave_thin_record(L, bins, k, plan.whole, plan.comp, m1, ksum, psum,
                                                               a.target_cdf, a.target_scalars, list, count, lane);
                if (lane < count) a.out[q + (uint64_t)list[lane] * a.n] = rec;
            }
            wave_sync_lds();  // wh and the scratch are written again for the next group or replicate
        }
    }
}

}  // namespace

hipError_t launch_thin(const ThinArgs& a, hipStream_t stream) {
    ThinArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = thin_waves(a.bins, a.table_slots, &lds);
    // (the kernel indexes its LDS, its groups and the records by these: refuse a block that does not agree with the plan)
    if (lds > kPassLdsMax || a.scratch_words != cohort_scratch_words(a.bins, a.table_slots) || a.n_targets < 1u ||
        a.n_targets > kMaxCohortTargets || a.n_groups < 1u || a.n_groups > a.n_targets ||
        a.group_offset[a.n_groups] > a.n_targets || !a.n || !a.reps_per_block || a.bins < 2u || !a.rid_stride || !a.m)
        return hipErrorInvalidValue;
    for (uint32_t g = 0; g < a.n_groups; ++g)
        if (a.group_offset[g] > a.group_offset[g + 1u]) return hipErrorInvalidValue;
    for (uint32_t j = 0; j < a.group_offset[a.n_groups]; ++j)
        if (a.group_targets[j] >= a.n_targets) return hipErrorInvalidValue;
    const uint32_t blocks = (a.n + a.reps_per_block - 1u) / a.reps_per_block;
    return hipLaunchKernel((const void*)ssa_thin, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
