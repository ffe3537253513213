// ssa_select_draws.hpp — the host side of the select over thinning draws (ecdna_ssa_ctx_select_draws and
// ecdna_ssa_ctx_select_draws_digits; thinned select mapping v1, include/ecdna_ssa.h): the validation of the call's
// arguments (ecdna_ssa_ctx_accept_draws' block without threshold rows, routed through accept_draws::invalid, then the
// 32-bit bound of the keys and the rank rules of ecdna_ssa_select_t), the byte counts of the call's buffers, and the
// block a context remembers its keys for. The grouping and the LDS plan are accept_draws::plan's. No HIP runtime call
// and nothing of the API, so all of it is checked on a machine without a GPU (tests/native/select_draws_check.cpp,
// tests/test_select_draws_native.py).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ecdna_ssa.h"
#include "ssa_accept_draws.hpp"
#include "ssa_select.hpp"

namespace ecdna {
namespace select_draws {

// The keys of a call: one per (replicate, draw of the range) and distance. The digit pass indexes them with 32 bits.
inline uint64_t n_keys(uint64_t n_replicates, uint32_t n_draws) { return n_replicates * n_draws; }

// What is wrong with the block, as the message of ECDNA_E_INVALID, which names the field; "" for a block the engine
// takes. Everything ecdna_ssa_ctx_accept_draws refuses, with its messages, except that the block has no threshold rows;
// the arguments are accept_draws::invalid's.
inline std::string invalid(uint32_t hist_bins, uint32_t keep_cells, uint32_t store_T, uint64_t n_replicates,
                           const ecdna_ssa_accept_draws_t& a) {
    const std::string bad = accept_draws::invalid(hist_bins, keep_cells, store_T, n_replicates, a, true);
    if (!bad.empty()) return bad;
    if (n_keys(n_replicates, a.n_draws) >= (1ull << 32))
        return "select_draws: n_replicates x n_draws = " + std::to_string(n_keys(n_replicates, a.n_draws)) +
               " must be < 2^32 (narrow the draw range)";
    return "";
}

// The rank rules of ecdna_ssa_select_t and the rules of ecdna_ssa_ctx_select_digits for one pass (ssa_select.hpp), under
// the names of this call's arguments.
inline std::string invalid_ranks(uint32_t n_ranks, const uint64_t* ranks, const double* fractions) {
    return select::invalid_ranks("select_draws", n_ranks, ranks, fractions);
}
inline std::string invalid_pass(uint32_t pass, uint32_t n_prefixes, const void* prefixes, const void* out_hist) {
    return select::invalid_pass("select_draws_digits", pass, n_prefixes, prefixes, out_hist);
}

// The bytes of the call's own buffers: the keys [4][n x n_draws] u64 (2.1 GB at n = 2^20 and 64 draws) and one pass's
// histogram [4][kMaxSelectGroups][256] u64; the target CDFs and scalars are accept_draws'.
inline uint64_t keys_bytes(uint64_t n_replicates, uint32_t n_draws) {
    return (uint64_t)select::kDistances * n_keys(n_replicates, n_draws) * sizeof(uint64_t);
}
inline uint64_t hist_words() { return (uint64_t)select::kDistances * kMaxSelectGroups * select::kDigits; }
inline uint64_t hist_bytes() { return hist_words() * sizeof(uint64_t); }
inline uint64_t cdf_bytes(uint32_t n_targets, uint32_t bins) { return accept_draws::cdf_bytes(n_targets, bins); }
inline uint64_t scalars_bytes(uint32_t n_targets) { return accept_draws::scalars_bytes(n_targets); }

// The block a context made its keys for: the fields that decide a key, and copies of what the block points to. A pass
// above 0 of ecdna_ssa_ctx_select_draws_digits reads the keys only when its block is the same one.
struct Block {
    uint32_t timepoints = 0, n_targets = 0, first_draw = 0, n_draws = 0;
    uint64_t timepoint_mask = 0;
    std::vector<uint64_t> target_hists;   // [n_targets][bins]
    std::vector<uint32_t> sample_cells;   // [n_targets]
};
// (of a block invalid() takes)
inline Block remember(const ecdna_ssa_accept_draws_t& a, uint32_t hist_bins) {
    Block b;
    b.timepoints = a.timepoints;
    b.n_targets = a.n_targets;
    b.first_draw = a.first_draw;
    b.n_draws = a.n_draws;
    b.timepoint_mask = a.timepoint_mask;
    b.target_hists.assign(a.target_hists, a.target_hists + (uint64_t)a.n_targets * hist_bins);
    b.sample_cells.assign(a.sample_cells, a.sample_cells + a.n_targets);
    return b;
}
inline bool same(const Block& b, const ecdna_ssa_accept_draws_t& a, uint32_t hist_bins) {
    if (b.timepoints != a.timepoints || b.n_targets != a.n_targets || b.first_draw != a.first_draw ||
        b.n_draws != a.n_draws || b.timepoint_mask != a.timepoint_mask ||
        b.target_hists.size() != (uint64_t)a.n_targets * hist_bins)
        return false;
    for (uint64_t j = 0; j < b.target_hists.size(); ++j)
        if (b.target_hists[j] != a.target_hists[j]) return false;
    for (uint32_t t = 0; t < a.n_targets; ++t)
        if (b.sample_cells[t] != a.sample_cells[t]) return false;
    return true;
}

}  // namespace select_draws
}  // namespace ecdna
