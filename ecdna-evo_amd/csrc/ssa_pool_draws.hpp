// ssa_pool_draws.hpp — the host side of the pooling over thinning draws (ecdna_ssa_ctx_pool_draws; thinned pooling
// mapping v1, include/ecdna_ssa.h): the validation of the call's arguments (ecdna_ssa_ctx_accept_draws' block, routed
// through accept_draws::invalid, then the threshold row and the outputs), the two groupings of the targets — the
// verdict's, which is accept_draws::plan under the block's mask, and the pooling's, which is accept_draws::plan with
// mask 0: a held-out target is pooled too — the LDS plan (ssa_thin's plus one [bins] u32 accumulator per wave) and
// the byte counts of the call's buffers. No HIP runtime call and nothing of the API, so all of it is checked on a machine
// without a GPU (tests/native/pool_draws_check.cpp, tests/test_pool_draws_native.py).
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/ecdna_ssa.h"
#include "ssa_accept_draws.hpp"
#include "ssa_launch.h"
#include "ssa_thin.hpp"

namespace ecdna {
namespace pool_draws {

// What is wrong with the call, as the message of ECDNA_E_INVALID, which names the field; "" for a call the engine
// takes. Everything ecdna_ssa_ctx_accept_draws refuses, with its messages, comes first; the arguments are
// accept_draws::invalid's and the call's own.
inline std::string invalid(uint32_t hist_bins, uint32_t keep_cells, uint32_t store_T, uint64_t n_replicates,
                           const ecdna_ssa_accept_draws_t& a, uint32_t threshold, const void* out_thinned,
                           const void* out_kept) {
    const std::string bad = accept_draws::invalid(hist_bins, keep_cells, store_T, n_replicates, a);
    if (!bad.empty()) return bad;
    if (threshold >= a.n_thresholds)
        return "pool_draws.threshold must be < accept_draws.n_thresholds = " + std::to_string(a.n_thresholds);
    if (!out_thinned && !out_kept) return "pool_draws.out_thinned and pool_draws.out_kept are both NULL";
    return "";
}

// The pass's LDS plan: thin::lds_plan under this pass's waves rule (the wave's accumulator behind the table).
inline thin::LdsPlan lds_plan(uint32_t bins, uint32_t max_mp) { return thin::lds_plan(bins, max_mp, pool_draws_waves); }

// The call's tables, as PoolDrawsArgs carries them. verdict: the grouping ecdna_ssa_ctx_accept_draws makes of the same
// block, so the verdict is that call's. pool: the same grouping with mask 0 — every slot takes part: on the keep store
// the targets grouped by m1 whatever the mask, on the timepoint store one group of one target per slice. lds: for the
// largest number of positions any group of either picks (the pooling's, which holds every group of the verdict's):
// ssa_thin's per-wave layout and the wave's accumulator behind the table (ssa_launch.h pool_draws_wave_words).
struct Plan {
    accept_draws::Plan verdict, pool;
    thin::LdsPlan lds{};
};
inline Plan plan(uint32_t bins, uint32_t keep_cells, bool timepoints, uint32_t n_targets, const uint32_t* sample_cells,
                 uint64_t timepoint_mask) {
    Plan p;
    p.verdict = accept_draws::plan(bins, keep_cells, timepoints, n_targets, sample_cells, timepoint_mask);
    p.pool = accept_draws::plan(bins, keep_cells, timepoints, n_targets, sample_cells, 0ull);
    p.lds = lds_plan(bins, p.pool.max_mp);
    return p;
}

// The bytes of the call's own buffers: the pooled arrays, thinned [n_targets][n_sets][bins] then kept
// [n_slices][n_sets][bins], u64; the target CDFs and scalars are accept_draws'.
inline uint64_t thinned_words(uint32_t n_targets, uint32_t n_sets, uint32_t bins) {
    return (uint64_t)n_targets * n_sets * bins;
}
inline uint64_t kept_words(uint32_t n_slices, uint32_t n_sets, uint32_t bins) {
    return (uint64_t)n_slices * n_sets * bins;
}
inline uint64_t pooled_bytes(uint32_t n_targets, uint32_t n_slices, uint32_t n_sets, uint32_t bins) {
    return (thinned_words(n_targets, n_sets, bins) + kept_words(n_slices, n_sets, bins)) * sizeof(uint64_t);
}
inline uint64_t cdf_bytes(uint32_t n_targets, uint32_t bins) { return accept_draws::cdf_bytes(n_targets, bins); }
inline uint64_t scalars_bytes(uint32_t n_targets) { return accept_draws::scalars_bytes(n_targets); }

}  // namespace pool_draws
}  // namespace ecdna
