// ssa_keep.hpp — the host side of the keep block (ecdna_ssa_keep_t, keep mapping v1, include/ecdna_ssa.h): the block's
// validation, the bytes the kept samples take, and the map from a replicate's global id to its index in the call
// (ecdna_ssa_ctx_download_kept). No HIP runtime call and nothing of the API, so all of it is checked on a machine
// without a GPU (tests/native/keep_check.cpp, tests/test_keep_native.py).
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/ecdna_ssa.h"

namespace ecdna {
namespace keep {

constexpr uint32_t kMaxKeepCells = 4096;  // kMaxSubsampleCells: the sample is subsample mapping v1's

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

// Bytes of the kept samples of a run: [n][m] u16 cells and [n] headers (at least one replicate's, as the other
// run-sized buffers).
inline uint64_t cells_bytes(uint64_t n, uint32_t m) { return (n ? n : 1u) * (uint64_t)m * sizeof(uint16_t); }
inline uint64_t headers_bytes(uint64_t n) { return (n ? n : 1u) * sizeof(ecdna_kept_t); }

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
}  // namespace ecdna
