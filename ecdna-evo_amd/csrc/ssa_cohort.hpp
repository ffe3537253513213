// ssa_cohort.hpp — the host side of the cohort block (ecdna_ssa_cohort_t, cohort mapping v1, include/ecdna_ssa.h): the
// block's validation, the grouping of the targets by distinct sample size, and the LDS plan of the cohort pass
// (ssa_cohort.hip). No HIP runtime call and nothing of the API, so all of it is checked on a machine without a GPU
// (tests/native/cohort_check.cpp, tests/test_cohort_native.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ecdna_ssa.h"
#include "ssa_launch.h"

namespace ecdna {
namespace cohort {

// What is wrong with a cohort block beside a run's (already validated) parameters, extension and passage blocks, as the
// message of ECDNA_E_INVALID, which names the field; "" for a block the engine takes. Reads host memory only.
inline std::string invalid(const ecdna_ssa_params_t& p, const ecdna_ssa_ext_t* ext, const ecdna_ssa_passages_t* pas,
                           const ecdna_ssa_cohort_t& co) {
    if (co.struct_size != sizeof(ecdna_ssa_cohort_t)) return "cohort.struct_size must be sizeof(ecdna_ssa_cohort_t)";
    if (co.reserved) return "cohort.reserved must be 0";
    if (co.n_targets < 1u || co.n_targets > kMaxCohortTargets) return "cohort.n_targets must be in [1, 64]";
    if (!co.target_hists) return "cohort.target_hists is NULL";
    if (!(p.flags & ECDNA_FLAG_REP_STATS)) return "cohort needs ECDNA_FLAG_REP_STATS in params.flags";
    if (pas)
        return "cohort: passages must be NULL (cohorts of longitudinal targets are a different feature)";
    if (ext && ext->snapshot_stats)
        return "cohort: ext.snapshot_stats must be 0 (cohorts of longitudinal targets are a different feature)";
    for (uint32_t t = 0; t < co.n_targets; ++t) {
        const uint64_t* h = co.target_hists + (uint64_t)t * p.hist_bins;
        if (std::all_of(h, h + p.hist_bins, [](uint64_t x) { return x == 0; }))
            return "cohort.target_hists[" + std::to_string(t) + "] is empty";
    }
    for (uint32_t t = 0; co.sample_cells && t < co.n_targets; ++t)
        if (co.sample_cells[t] < 1u || co.sample_cells[t] > kMaxSubsampleCells)
            return "cohort.sample_cells[" + std::to_string(t) + "] must be in [1, 4096]";
    return "";
}

// The targets grouped by distinct sample size, the groups in order of first appearance and a group's targets ascending:
// group g has sample size m[g] and the targets targets[offset[g] .. offset[g + 1]). The pass draws one sample per group.
// n_groups = 0 without sample sizes. max_m: the largest sample size, which sizes the wave's table of drawn positions.
struct Groups {
    uint32_t n_groups = 0, max_m = 0;
    uint32_t m[kMaxCohortTargets] = {};
    uint32_t offset[kMaxCohortTargets + 1] = {};
    uint32_t targets[kMaxCohortTargets] = {};
};
inline Groups group_by_sample_size(const uint32_t* sample_cells, uint32_t n_targets) {
    Groups g;
    if (!sample_cells) return g;
    const uint32_t P = std::min(n_targets, kMaxCohortTargets);
    uint32_t group_of[kMaxCohortTargets] = {};
    for (uint32_t t = 0; t < P; ++t) {
        uint32_t j = 0;
        while (j < g.n_groups && g.m[j] != sample_cells[t]) ++j;
        if (j == g.n_groups) g.m[g.n_groups++] = sample_cells[t];
        group_of[t] = j;
        g.max_m = std::max(g.max_m, sample_cells[t]);
    }
    uint32_t at = 0;
    for (uint32_t j = 0; j < g.n_groups; ++j) {
        g.offset[j] = at;
        for (uint32_t t = 0; t < P; ++t)
            if (group_of[t] == j) g.targets[at++] = t;
    }
    g.offset[g.n_groups] = at;
    return g;
}

// The cohort pass's LDS plan for a run of `bins` histogram bins and bag_k bin counters (0: row store) whose largest
// sample size is max_m (0: no samples): waves per workgroup, the table's slots and the dynamic LDS (ssa_launch.h).
struct LdsPlan {
    uint32_t waves, table_slots, scratch_words;
    size_t lds_bytes;
};
inline LdsPlan lds_plan(uint32_t bins, uint32_t bag_k, uint32_t max_m) {
    LdsPlan l{};
    l.table_slots = max_m ? subsample_table_slots(max_m) : 0u;
    l.scratch_words = cohort_scratch_words(bins, l.table_slots);
    l.waves = cohort_waves(bins, bag_k, l.table_slots, &l.lds_bytes);
    return l;
}

}  // namespace cohort
}  // namespace ecdna
