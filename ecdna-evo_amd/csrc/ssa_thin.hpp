// ssa_thin.hpp — the host side of the sized rescore (ecdna_ssa_rescore_t, ecdna_ssa_ctx_rescore_sized and
// _rescore_timepoints_sized; thinning mapping v1, include/ecdna_ssa.h): the validation of the two calls' arguments, the
// grouping of the targets by (measured cells, draw index), the thinning stream's tag, and the LDS plan of the thinning
// pass (ssa_thin.hip). No HIP runtime call and nothing of the API, so all of it is checked on a machine without a GPU
// (tests/native/thin_check.cpp, tests/test_thin_native.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ecdna_ssa.h"
#include "ssa_launch.h"

namespace ecdna {
namespace thin {

constexpr uint32_t kMaxDraw = kThinDraws - 1u;  // 63: the draw index d takes 6 bits
constexpr uint32_t kSampleTag = 0xC0000000u; // the sampling passes' tag (ssa_sampledraw.hpp kSubTag)
constexpr uint32_t kThinFlag = 0x20000000u;  // bit 29: the sampling passes keep it clear

// Counter word 1 of thinning draw block t is stream_tag(...) | t, t < 2^10: the tag of the stream the slice's own sample
// was drawn on (snapshot_plus_one = 0 for the end of the run and for a passage phase, s + 1 for snapshot s < 64), the
// thinning flag, and the draw index d <= kMaxDraw in bits 10-15. t takes bits 0-9, d bits 10-15, the snapshot field bits
// 16-22, the flag bit 29, the tag bits 30-31: the fields never meet.
// draw_tag: a slice's tag stream_tag(field, 0) with the draw index set, as the passes over a range of draws form it.
constexpr uint32_t draw_tag(uint32_t slice_tag, uint32_t d) { return slice_tag | (d << 10); }
constexpr uint32_t stream_tag(uint32_t snapshot_plus_one, uint32_t d) {
    return draw_tag(kSampleTag | (snapshot_plus_one << 16) | kThinFlag, d);
}

inline bool empty_row(const uint64_t* h, uint32_t bins) {
    return std::all_of(h, h + bins, [](uint64_t x) { return x == 0; });
}

// What is wrong with the block of ecdna_ssa_ctx_rescore_sized on a context of hist_bins bins that keeps keep_cells cells
// per replicate, as the message of ECDNA_E_INVALID, which names the field; "" for a block the engine takes. Reads host
// memory only.
inline std::string invalid(uint32_t hist_bins, uint32_t keep_cells, const ecdna_ssa_rescore_t& r) {
    if (r.struct_size != sizeof(ecdna_ssa_rescore_t))
        return "rescore_sized.struct_size must be sizeof(ecdna_ssa_rescore_t)";
    if (r.reserved) return "rescore_sized.reserved must be 0";
    if (r.n_targets < 1u || r.n_targets > kMaxCohortTargets) return "rescore_sized.n_targets must be in [1, 64]";
    if (!r.target_hists) return "rescore_sized.target_hists is NULL";
    for (uint32_t t = 0; t < r.n_targets; ++t)
        if (empty_row(r.target_hists + (uint64_t)t * hist_bins, hist_bins))
            return "rescore_sized.target_hists[" + std::to_string(t) + "] is empty";
    for (uint32_t t = 0; r.sample_cells && t < r.n_targets; ++t)
        if (r.sample_cells[t] < 1u || r.sample_cells[t] > keep_cells)
            return "rescore_sized.sample_cells[" + std::to_string(t) + "] must be in [1, keep_cells = " +
                   std::to_string(keep_cells) + "]: a target with more measured cells than were kept cannot be served";
    for (uint32_t t = 0; r.sample_draws && t < r.n_targets; ++t)
        if (r.sample_draws[t] > kMaxDraw)
            return "rescore_sized.sample_draws[" + std::to_string(t) + "] must be in [0, 63]";
    return "";
}

// Likewise the arguments of ecdna_ssa_ctx_rescore_timepoints_sized on a context of T timepoints.
inline std::string invalid_timepoints(uint32_t hist_bins, uint32_t keep_cells, uint32_t T, const uint64_t* target_hists,
                                      const uint32_t* sample_cells, uint32_t draw) {
    if (!target_hists) return "rescore_timepoints_sized.target_hists is NULL";
    for (uint32_t t = 0; t < T; ++t)
        if (empty_row(target_hists + (uint64_t)t * hist_bins, hist_bins))
            return "rescore_timepoints_sized.target_hists[" + std::to_string(t) + "] is empty";
    for (uint32_t t = 0; sample_cells && t < T; ++t)
        if (sample_cells[t] < 1u || sample_cells[t] > keep_cells)
            return "rescore_timepoints_sized.sample_cells[" + std::to_string(t) + "] must be in [1, keep_cells = " +
                   std::to_string(keep_cells) + "]: a target with more measured cells than were kept cannot be served";
    if (draw > kMaxDraw) return "rescore_timepoints_sized.draw must be in [0, 63]";
    return "";
}

// The targets grouped by (measured cells m1, draw index d), the groups in order of first appearance and a group's
// targets ascending: group g has m[g], d[g] and the targets targets[offset[g] .. offset[g + 1]). The pass draws one
// thinned sample per group. draws == nullptr: every d is 0. max_mp: the largest number of positions a group can pick
// from a kept sample of at most keep_cells cells, min(m1, keep_cells - m1) — it sizes the wave's table of drawn
// positions and never exceeds keep_cells / 2.
struct Groups {
    uint32_t n_groups = 0, max_mp = 0;
    uint32_t m[kMaxCohortTargets] = {};
    uint32_t d[kMaxCohortTargets] = {};
    uint32_t offset[kMaxCohortTargets + 1] = {};
    uint32_t targets[kMaxCohortTargets] = {};
};
inline Groups group_by_size_and_draw(const uint32_t* sample_cells, const uint32_t* draws, uint32_t n_targets,
                                     uint32_t keep_cells) {
    Groups g;
    if (!sample_cells) return g;
    const uint32_t P = std::min(n_targets, kMaxCohortTargets);
    uint32_t group_of[kMaxCohortTargets] = {};
    for (uint32_t t = 0; t < P; ++t) {
        const uint32_t m1 = sample_cells[t], d = draws ? draws[t] : 0u;
        uint32_t j = 0;
        while (j < g.n_groups && (g.m[j] != m1 || g.d[j] != d)) ++j;
        if (j == g.n_groups) {
            g.m[j] = m1;
            g.d[j] = d;
            ++g.n_groups;
        }
        group_of[t] = j;
        g.max_mp = std::max(g.max_mp, std::min(m1, keep_cells > m1 ? keep_cells - m1 : 0u));
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

// The thinning pass's LDS plan for `bins` histogram bins when a group picks at most max_mp positions (0: every target
// takes the whole kept sample): waves per workgroup, the table's slots and the dynamic LDS (ssa_launch.h). waves: the
// pass's rule for its waves and bytes — thin_waves, or pool_draws_waves for the pass that keeps an accumulator behind
// the table; lds_bytes / waves is the per-wave size.
struct LdsPlan {
    uint32_t waves, table_slots, scratch_words;
    size_t lds_bytes;
};
inline LdsPlan lds_plan(uint32_t bins, uint32_t max_mp,
                        uint32_t (*waves)(uint32_t, uint32_t, size_t*) = thin_waves) {
    LdsPlan l{};
    l.table_slots = max_mp ? subsample_table_slots(max_mp) : 0u;
    l.scratch_words = cohort_scratch_words(bins, l.table_slots);
    l.waves = waves(bins, l.table_slots, &l.lds_bytes);
    return l;
}

}  // namespace thin
}  // namespace ecdna
