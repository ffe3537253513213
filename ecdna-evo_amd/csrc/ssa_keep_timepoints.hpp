// ssa_keep_timepoints.hpp — the host side of the timepoint keep block (ecdna_ssa_keep_timepoints_t, timepoint keep
// mapping v1, include/ecdna_ssa.h): the block's validation, the number of timepoints T of a context, and the bytes the
// kept samples take. No HIP runtime call and nothing of the API, so all of it is checked on a machine without a GPU
// (tests/native/timepoint_keep_check.cpp, tests/test_timepoint_keep_native.py).
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/ecdna_ssa.h"

namespace ecdna {
namespace keep_timepoints {

constexpr uint32_t kMaxKeepCells = 4096;  // kMaxSubsampleCells: the samples are subsample mapping v1's

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
    if (k.keep_cells < 1u || k.keep_cells > kMaxKeepCells) return "keep_timepoints.keep_cells must be in [1, 4096]";
    if (!(p.flags & ECDNA_FLAG_REP_STATS)) return "keep_timepoints needs ECDNA_FLAG_REP_STATS in params.flags";
    if (timepoints(p, ext, pas) == 0u)
        return "keep_timepoints needs timepoints: a passage block (passages), or snapshots with ext.snapshot_stats";
    // (the kept sample of phase g founds phase g + 1: another size on the same stream would be a different sample)
    if (pas && k.keep_cells != pas->passage_cells)
        return "keep_timepoints.keep_cells must equal passages.passage_cells";
    return "";
}

// Bytes of the kept samples of a run: [T][n][m] u16 cells and [T][n] headers (at least one replicate's, as the other
// run-sized buffers): T * n * (2 m + 8).
inline uint64_t cells_bytes(uint32_t T, uint64_t n, uint32_t m) {
    return (uint64_t)T * (n ? n : 1u) * (uint64_t)m * sizeof(uint16_t);
}
inline uint64_t headers_bytes(uint32_t T, uint64_t n) { return (uint64_t)T * (n ? n : 1u) * sizeof(ecdna_kept_t); }
inline uint64_t bytes(uint32_t T, uint64_t n, uint32_t m) { return cells_bytes(T, n, m) + headers_bytes(T, n); }

}  // namespace keep_timepoints
}  // namespace ecdna
