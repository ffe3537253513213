// keep_check.cpp — the host side of the keep block (ecdna-evo_amd/csrc/ssa_keep.hpp) on the CPU, for
// tests/test_keep_native.py: the map from a global replicate id to its index in the call, the bytes the kept samples
// take and every branch of the block's validation. Built for the host alone, with the address and undefined-behaviour
// sanitizers.
//
//   keep_check index first stride n id0 id1 ...   prints per id its index in the call, or "no"
//   keep_check bytes n m                           prints "cells <bytes> headers <bytes>"
//   keep_check validate                            checks every validation branch; prints "validate ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ssa_keep.hpp"

namespace kp = ecdna::keep;

static uint64_t u64(const char* s) { return std::strtoull(s, nullptr, 10); }

static int print_index(int argc, char** argv) {
    if (argc < 5) return 2;
    const uint64_t first = u64(argv[2]), stride = u64(argv[3]), n = u64(argv[4]);
    for (int i = 5; i < argc; ++i) {
        uint64_t index = ~0ull;
        if (kp::index_of(u64(argv[i]), first, stride, n, &index))
            std::printf("%llu\n", (unsigned long long)index);
        else
            std::printf("no\n");
    }
    return 0;
}

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

static int check_validate() {
    ecdna_ssa_params_t p{};
    p.hist_bins = 5;
    p.flags = ECDNA_FLAG_REP_STATS;
    ecdna_ssa_keep_t good{};
    good.struct_size = sizeof good;
    good.keep_cells = 200;
    ecdna_ssa_passages_t pas{};
    int bad = 0;
    bad += expect(kp::invalid(p, nullptr, good), nullptr, "a good block");
    for (uint32_t m : {1u, 64u, 65u, 4096u}) {
        ecdna_ssa_keep_t k = good;
        k.keep_cells = m;
        bad += expect(kp::invalid(p, nullptr, k), nullptr, "a sample size in range");
    }
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        ecdna_ssa_keep_t k = good;
        k.struct_size = size;
        bad += expect(kp::invalid(p, nullptr, k), "struct_size", "struct_size");
    }
    for (uint32_t m : {0u, 4097u, 0xffffffffu}) {
        ecdna_ssa_keep_t k = good;
        k.keep_cells = m;
        bad += expect(kp::invalid(p, nullptr, k), "keep_cells", "keep_cells out of range");
    }
    for (uint64_t r : {1ull, 1ull << 40}) {
        ecdna_ssa_keep_t k = good;
        k.reserved = r;
        bad += expect(kp::invalid(p, nullptr, k), "reserved", "reserved");
    }
    ecdna_ssa_params_t q = p;
    q.flags = 0;
    bad += expect(kp::invalid(q, nullptr, good), "REP_STATS", "flags");
    bad += expect(kp::invalid(p, &pas, good), "passages", "a passage block");
    // params.subsample_cells and a target keep their meaning beside the block
    q = p;
    q.subsample_cells = 7;
    bad += expect(kp::invalid(q, nullptr, good), nullptr, "subsample_cells beside the block");
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "index") == 0) return print_index(argc, argv);
    if (argc == 4 && std::strcmp(argv[1], "bytes") == 0) {
        std::printf("cells %llu headers %llu\n", (unsigned long long)kp::cells_bytes(1u, u64(argv[2]), (uint32_t)u64(argv[3])),
                    (unsigned long long)kp::headers_bytes(1u, u64(argv[2])));
        return 0;
    }
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    std::fprintf(stderr, "usage: keep_check index first stride n id ... | bytes n m | validate\n");
    return 2;
}
