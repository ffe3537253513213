// ssa_keep.hpp — the host side of the kept samples: the keep block (ecdna_ssa_keep_t, keep mapping v1,
// include/ecdna_ssa.h) and the timepoint keep block (ecdna_ssa_keep_timepoints_t, timepoint keep mapping v1). Each
// block's validation, the number of timepoints T of a context, the bytes the kept samples take, and the map from a
// replicate's global id to its index in the call (ecdna_ssa_ctx_download_kept, _download_kept_timepoints). No HIP
// runtime call and nothing of the API, so all of it is checked on a machine without a GPU (tests/native/keep_check.cpp,
// tests/native/timepoint_keep_check.cpp; tests/test_keep_native.py, tests/test_timepoint_keep_native.py).
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/ecdna_ssa.h"

namespace ecdna {
namespace keep {

constexpr uint32_t kMaxKeepCells = 4096;  // kMaxSubsampleCells: the samples are subsample mapping v1's

// What is wrong with a keep block beside a run's (already validated) parameters and passage block, as the message of
// ECDNA_E_INVALID, which names the field; "" for a block the engine takes. Reads host memory only.
inline std::string invalid(const ecdna_ssa_params_t& p, const ecdna_ssa_passages_t* pas, const ecdna_ssa_keep_t& k) {
    if (k.struct_size != sizeof(ecdna_ssa_keep_t)) return "keep.struct_size must be sizeof(ecdna_ssa_keep_t)";
    if (k.reserved) return "keep.reserved must be 0";
    if (k.keep_cells < 1u || k.keep_cells > kMaxKeepCells) return "keep.keep_cells must be in [1, 4096]";
    if (!(p.flags & ECDNA_FLAG_REP_STATS)) return "keep needs ECDNA_FLAG_REP_STATS in params.flags";
    if (pas) return "keep: passages must be NULL (kept samples of every phase are a different feature)";
    return "";
}

// Bytes of the kept samples of a run: [T][n][m] u16 cells and [T][n] headers (at least one replicate's, as the other
// run-sized buffers): T * n * (2 m + 8). The keep block's are T = 1.
inline uint64_t cells_bytes(uint32_t T, uint64_t n, uint32_t m) {
    return (uint64_t)T * (n ? n : 1u) * (uint64_t)m * sizeof(uint16_t);
}
inline uint64_t headers_bytes(uint32_t T, uint64_t n) { return (uint64_t)T * (n ? n : 1u) * sizeof(ecdna_kept_t); }
inline uint64_t bytes(uint32_t T, uint64_t n, uint32_t m) { return cells_bytes(T, n, m) + headers_bytes(T, n); }

// The index in the call of the replicate with global id `id`: the call's replicates are first + i * stride, i < n
// (stride >= 1). False for an id that is not one of them.
inline bool index_of(uint64_t id, uint64_t first, uint64_t stride, uint64_t n, uint64_t* index) {
    if (id < first || stride == 0) return false;
    const uint64_t d = id - first;
    if (d % stride) return false;
    const uint64_t i = d / stride;
    if (i >= n) return false;
    *index = i;
    return true;
}

}  // namespace keep

namespace keep_timepoints {

// The timepoints of a context: the growth phases of a passage run, else the snapshots of a run with snapshot
// statistics; 0 for a context that has neither.
inline uint32_t timepoints(const ecdna_ssa_params_t& p, const ecdna_ssa_ext_t* ext, const ecdna_ssa_passages_t* pas) {
    if (pas) return pas->n_passages;
    return (ext && ext->snapshot_stats) ? p.n_snapshots : 0u;
}

// What is wrong with a timepoint keep block beside a run's (already validated) parameters, extension and passage
// blocks, as the message of ECDNA_E_INVALID, which names the field; "" for a block the engine takes. Reads host memory
// only.
inline std::string invalid(const ecdna_ssa_params_t& p, const ecdna_ssa_ext_t* ext, const ecdna_ssa_passages_t* pas,
                           const ecdna_ssa_keep_timepoints_t& k) {
    if (k.struct_size != sizeof(ecdna_ssa_keep_timepoints_t))
        return "keep_timepoints.struct_size must be sizeof(ecdna_ssa_keep_timepoints_t)";
    if (k.reserved) return "keep_timepoints.reserved must be 0";
    if (k.keep_cells < 1u || k.keep_cells > keep::kMaxKeepCells)
        return "keep_timepoints.keep_cells must be in [1, 4096]";
    if (!(p.flags & ECDNA_FLAG_REP_STATS)) return "keep_timepoints needs ECDNA_FLAG_REP_STATS in params.flags";
    if (timepoints(p, ext, pas) == 0u)
        return "keep_timepoints needs timepoints: a passage block (passages), or snapshots with ext.snapshot_stats";
    // (the kept sample of phase g founds phase g + 1: another size on the same stream would be a different sample)
    if (pas && k.keep_cells != pas->passage_cells)
        return "keep_timepoints.keep_cells must equal passages.passage_cells";
    return "";
}

}  // namespace keep_timepoints
}  // namespace ecdna
