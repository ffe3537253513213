// timepoint_keep_check.cpp — the host side of the timepoint keep block (ecdna-evo_amd/csrc/ssa_keep.hpp) on
// the CPU, for tests/test_timepoint_keep_native.py: the timepoints of a context, the bytes the kept samples take and
// every branch of the block's validation. Built for the host alone, with the address and undefined-behaviour
// sanitizers.
//
//   timepoint_keep_check bytes T n m     prints "cells <bytes> headers <bytes> all <bytes>"
//   timepoint_keep_check validate        checks T and every validation branch; prints "validate ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ssa_keep.hpp"

namespace kp = ecdna::keep;
namespace kt = ecdna::keep_timepoints;

static uint64_t u64(const char* s) { return std::strtoull(s, nullptr, 10); }

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

static int check_validate() {
    ecdna_ssa_params_t p{};
    p.hist_bins = 5;
    p.flags = ECDNA_FLAG_REP_STATS;
    p.n_snapshots = 3;
    ecdna_ssa_ext_t ext{};
    ext.struct_size = sizeof ext;
    ext.snapshot_stats = 1;
    ecdna_ssa_params_t pp = p;  // a passage run takes no snapshots
    pp.n_snapshots = 0;
    ecdna_ssa_passages_t pas{};
    pas.struct_size = sizeof pas;
    pas.n_passages = 4;
    pas.passage_cells = 200;
    ecdna_ssa_keep_timepoints_t good{};
    good.struct_size = sizeof good;
    good.keep_cells = 200;
    int bad = 0;
    // T: the growth phases, else the snapshots under snapshot_stats, else none
    bad += kt::timepoints(p, &ext, nullptr) != 3u;
    bad += kt::timepoints(pp, nullptr, &pas) != 4u;
    bad += kt::timepoints(p, nullptr, nullptr) != 0u;
    ecdna_ssa_ext_t off = ext;
    off.snapshot_stats = 0;
    bad += kt::timepoints(p, &off, nullptr) != 0u;
    if (bad) return std::fprintf(stderr, "timepoints\n"), 1;

    bad += expect(kt::invalid(p, &ext, nullptr, good), nullptr, "a good block beside snapshots");
    bad += expect(kt::invalid(pp, nullptr, &pas, good), nullptr, "a good block beside passages");
    for (uint32_t m : {1u, 64u, 65u, 4096u}) {
        ecdna_ssa_keep_timepoints_t k = good;
        k.keep_cells = m;
        bad += expect(kt::invalid(p, &ext, nullptr, k), nullptr, "a sample size in range");
        ecdna_ssa_passages_t q = pas;
        q.passage_cells = m;
        bad += expect(kt::invalid(pp, nullptr, &q, k), nullptr, "a sample size equal to passage_cells");
    }
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        ecdna_ssa_keep_timepoints_t k = good;
        k.struct_size = size;
        bad += expect(kt::invalid(p, &ext, nullptr, k), "keep_timepoints.struct_size", "struct_size");
    }
    for (uint64_t r : {1ull, 1ull << 40}) {
        ecdna_ssa_keep_timepoints_t k = good;
        k.reserved = r;
        bad += expect(kt::invalid(p, &ext, nullptr, k), "keep_timepoints.reserved", "reserved");
    }
    for (uint32_t m : {0u, 4097u, 0xffffffffu}) {
        ecdna_ssa_keep_timepoints_t k = good;
        k.keep_cells = m;
        bad += expect(kt::invalid(p, &ext, nullptr, k), "keep_timepoints.keep_cells", "keep_cells out of range");
    }
    ecdna_ssa_params_t q = p;
    q.flags = 0;
    bad += expect(kt::invalid(q, &ext, nullptr, good), "REP_STATS", "flags");
    // neither a passage block nor snapshot statistics: no block, the block off, no snapshots
    bad += expect(kt::invalid(p, nullptr, nullptr, good), "snapshot_stats", "no timepoints: no ext");
    bad += expect(kt::invalid(p, nullptr, nullptr, good), "passages", "no timepoints: names both");
    bad += expect(kt::invalid(p, &off, nullptr, good), "snapshot_stats", "no timepoints: snapshot_stats = 0");
    bad += expect(kt::invalid(pp, &ext, nullptr, good), "snapshot_stats", "no timepoints: no snapshots");
    // a passage block with another sample size
    for (uint32_t m : {199u, 201u, 1u}) {
        ecdna_ssa_keep_timepoints_t k = good;
        k.keep_cells = m;
        bad += expect(kt::invalid(pp, nullptr, &pas, k), "passage_cells", "keep_cells != passage_cells");
    }
    // ext->snapshot_subsample_cells keeps its meaning beside the block
    ecdna_ssa_ext_t sub = ext;
    sub.snapshot_subsample_cells = 7;
    bad += expect(kt::invalid(p, &sub, nullptr, good), nullptr, "snapshot_subsample_cells beside the block");
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "bytes") == 0) {
        const uint32_t T = (uint32_t)u64(argv[2]), m = (uint32_t)u64(argv[4]);
        const uint64_t n = u64(argv[3]);
        std::printf("cells %llu headers %llu all %llu\n", (unsigned long long)kp::cells_bytes(T, n, m),
                    (unsigned long long)kp::headers_bytes(T, n), (unsigned long long)kp::bytes(T, n, m));
        return 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    std::fprintf(stderr, "usage: timepoint_keep_check bytes T n m | validate\n");
    return 2;
}
