// ssa_accept_draws.hpp — the host side of the acceptance over repeated thinnings (ecdna_ssa_accept_draws_t,
// ecdna_ssa_ctx_accept_draws; thinned acceptance mapping v1, include/ecdna_ssa.h): the validation of the call's block,
// the per-slice grouping of the participating targets by measured cells (thin::group_by_size_and_draw with the draw
// held fixed), the LDS plan (ssa_thin's, for the call's largest m') and the byte counts of the call's buffers and of the
// records the loop it replaces allocates. No HIP runtime call and nothing of the API, so all of it is checked on a
// machine without a GPU (tests/native/accept_draws_check.cpp, tests/test_accept_draws_native.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ecdna_ssa.h"
#include "ssa_launch.h"
#include "ssa_thin.hpp"

namespace ecdna {
namespace accept_draws {

constexpr uint32_t kMaxDraws = kThinDraws;  // 64: the draw index takes 6 bits

#pragma GCC visibility push(hidden)  // (shared by the library's own units: not for its symbol table)
// Two rules every acceptance call has (ecdna_ssa_ctx_accept, _select, _select_digits, and the calls over this block),
// as the message of ECDNA_E_INVALID or "". who: the prefix the call's fields are named under.
// The timepoint mask: no bit at or above T; mask 0 stands for all T (all_timepoints).
inline uint64_t all_timepoints(uint32_t T) { return T >= 64u ? ~0ull : (1ull << T) - 1ull; }
inline std::string invalid_timepoint_mask(const std::string& who, uint64_t mask, uint32_t T) {
    if (mask & ~all_timepoints(T)) return who + ".timepoint_mask has bits at or above T = " + std::to_string(T);
    return "";
}
// The threshold rows: every threshold >= 0 and not NaN.
inline std::string invalid_threshold_rows(const std::string& who, uint32_t n, const ecdna_accept_threshold_t* rows) {
    for (uint32_t q = 0; q < n; ++q) {
        const ecdna_accept_threshold_t& t = rows[q];
        const double v[4] = {t.ks, t.mean_rel, t.entropy_rel, t.frequency_diff};
        const char* names[4] = {"ks", "mean_rel", "entropy_rel", "frequency_diff"};
        for (int k = 0; k < 4; ++k)
            if (!(v[k] >= 0.0))
                return who + ".thresholds[" + std::to_string(q) + "]." + names[k] +
                       " must be >= 0 (+inf switches it off) and not NaN";
    }
    return "";
}
#pragma GCC visibility pop

// What is wrong with the block on a context of hist_bins bins and n_replicates replicates, as the message of
// ECDNA_E_INVALID, which names the field; "" for a block the engine takes. keep_cells: the kept cells of the store the
// block names (a context without it: the largest any store keeps). store_T: the timepoints of the timepoint keep block,
// 0 for a context without it (the block is then refused for its state, not for n_targets). Reads host memory only.
// finds_thresholds: the call is ecdna_ssa_ctx_select_draws, whose block carries no threshold rows (ssa_select_draws.hpp):
// in the place of the threshold rules it must have none; every other rule and message is this call's.
inline std::string invalid(uint32_t hist_bins, uint32_t keep_cells, uint32_t store_T, uint64_t n_replicates,
                           const ecdna_ssa_accept_draws_t& a, bool finds_thresholds = false) {
    if (a.struct_size != sizeof(ecdna_ssa_accept_draws_t))
        return "accept_draws.struct_size must be sizeof(ecdna_ssa_accept_draws_t)";
    if (a.reserved) return "accept_draws.reserved must be 0";
    if (a.timepoints > 1u) return "accept_draws.timepoints must be 0 (the keep block) or 1 (the timepoint keep block)";
    if (a.n_targets < 1u || a.n_targets > kMaxCohortTargets) return "accept_draws.n_targets must be in [1, 64]";
    if (a.timepoints && store_T && a.n_targets != store_T)
        return "accept_draws.n_targets must be T = " + std::to_string(store_T) +
               " on the timepoint keep block: one target per timepoint";
    if (!a.target_hists) return "accept_draws.target_hists is NULL";
    for (uint32_t t = 0; t < a.n_targets; ++t)
        if (thin::empty_row(a.target_hists + (uint64_t)t * hist_bins, hist_bins))
            return "accept_draws.target_hists[" + std::to_string(t) + "] is empty";
    if (!a.sample_cells) return "accept_draws.sample_cells is NULL";
    for (uint32_t t = 0; t < a.n_targets; ++t)
        if (a.sample_cells[t] < 1u || a.sample_cells[t] > keep_cells)
            return "accept_draws.sample_cells[" + std::to_string(t) + "] must be in [1, keep_cells = " +
                   std::to_string(keep_cells) + "]: a target with more measured cells than were kept cannot be served";
    if (a.n_draws < 1u || a.n_draws > kMaxDraws) return "accept_draws.n_draws must be in [1, 64]";
    if (a.first_draw > kMaxDraws - a.n_draws) return "accept_draws.first_draw + n_draws must be <= 64";
    if (finds_thresholds) {
        if (a.n_thresholds) return "select_draws.n_thresholds must be 0: the call finds the thresholds";
        if (a.thresholds) return "select_draws.thresholds must be NULL: the call finds the thresholds";
    } else {
        if (a.n_thresholds < 1u || a.n_thresholds > kMaxAcceptRows)
            return "accept_draws.n_thresholds must be in [1, 32]";
        if (!a.thresholds) return "accept_draws.thresholds is NULL";
    }
    std::string bad = invalid_threshold_rows("accept_draws", a.n_thresholds, a.thresholds);
    // the acceptance's timepoints: the targets of the keep store, the slices of the timepoint store (== n_targets)
    if (bad.empty()) bad = invalid_timepoint_mask("accept_draws", a.timepoint_mask, a.n_targets);
    if (!bad.empty()) return bad;
    if (n_replicates >= (1ull << 32)) return "accept_draws: n_replicates must be < 2^32";
    return "";
}

// The call's tables: the Grouping AcceptDrawsArgs carries (ssa_launch.h), which the plan is — its base, so the call
// assigns it to the argument block — and the slices it is over. Keep store: one slice whose groups are the
// participating targets grouped by m1, in order of first appearance, a group's targets ascending. Timepoint store:
// slice t has one group of one target, t, and takes part when the mask names it. A target the mask leaves out is in no
// group: it is neither drawn nor scored. max_mp: the largest number of positions a group picks, which sizes the table
// of the LDS plan.
struct Plan : Grouping {
    uint32_t n_slices = 0, max_mp = 0;
    uint64_t slice_mask = 0;
    thin::LdsPlan lds{};
    Plan() : Grouping{} {}
    const Grouping& grouping() const { return *this; }
};
inline Plan plan(uint32_t bins, uint32_t keep_cells, bool timepoints, uint32_t n_targets, const uint32_t* sample_cells,
                 uint64_t timepoint_mask) {
    Plan p;
    const uint32_t P = std::min(n_targets, kMaxCohortTargets);
    const uint64_t all = all_timepoints(P);
    const uint64_t mask = timepoint_mask ? (timepoint_mask & all) : all;
    uint32_t at = 0;
    auto add = [&](const thin::Groups& g, uint32_t first_target, uint64_t take) {
        for (uint32_t j = 0; j < g.n_groups; ++j) {
            const uint32_t begin = at;
            for (uint32_t k = g.offset[j]; k < g.offset[j + 1u]; ++k)
                if ((take >> g.targets[k]) & 1ull) p.group_targets[at++] = first_target + g.targets[k];
            if (at == begin) continue;  // (none of the group's targets takes part)
            p.group_m[p.n_groups] = g.m[j];
            p.group_offset[p.n_groups++] = begin;
            p.max_mp = std::max(p.max_mp, std::min(g.m[j], keep_cells > g.m[j] ? keep_cells - g.m[j] : 0u));
        }
        p.group_offset[p.n_groups] = at;
    };
    if (!timepoints) {
        p.n_slices = 1;
        p.slice_mask = 1;
        add(thin::group_by_size_and_draw(sample_cells, nullptr, P, keep_cells), 0u, mask);
        p.slice_group[1] = p.n_groups;
    } else {
        p.n_slices = P;
        p.slice_mask = mask;
        for (uint32_t t = 0; t < P; ++t) {
            if ((mask >> t) & 1ull) add(thin::group_by_size_and_draw(sample_cells + t, nullptr, 1u, keep_cells), t, 1ull);
            p.slice_group[t + 1u] = p.n_groups;
        }
    }
    p.lds = thin::lds_plan(bins, p.max_mp);
    return p;
}

// The bytes of the call's own buffers, and of the records [slots][n] the loop of sized rescores it replaces allocates
// for the same draws (the keep store: every draw takes a target slot; the timepoint store: [T][n] rewritten per draw).
inline uint64_t passes_bytes(uint64_t n, uint32_t Q) { return n * Q; }
inline uint64_t sums_bytes(uint32_t Q, uint32_t n_sets) { return (uint64_t)Q * n_sets * sizeof(uint64_t); }
inline uint64_t cdf_bytes(uint32_t n_targets, uint32_t bins) { return (uint64_t)n_targets * bins * sizeof(double); }
inline uint64_t scalars_bytes(uint32_t n_targets) { return (uint64_t)n_targets * 3u * sizeof(double); }
inline uint64_t loop_record_bytes(uint64_t n, uint32_t slots) { return n * slots * sizeof(ecdna_rep_stats_t); }

}  // namespace accept_draws
}  // namespace ecdna
