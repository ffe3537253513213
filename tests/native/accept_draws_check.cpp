// accept_draws_check.cpp — the host side of the acceptance over repeated thinnings
// (ecdna-evo_amd/csrc/ssa_accept_draws.hpp) on the CPU, for tests/test_accept_draws_native.py: every branch of the
// call's validation, the per-slice grouping of the participating targets, the LDS plan at the limits and the byte
// counts. Built for the host alone, with the address and undefined-behaviour sanitizers.
//
//   accept_draws_check plan K S MASK m0 m1 ...  prints the plan at keep_cells = K for store S (0 keep, 1 timepoints) and
//                                               timepoint mask MASK (hex): "slices N mask M groups G max_mp X", then per
//                                               slice "slice s groups a b", per group "m <size> targets t t ..."
//   accept_draws_check lds                      checks the plan's LDS over bins x keep_cells; prints "lds ok" and the
//                                               plan at the limits
//   accept_draws_check bytes                    prints the byte counts of the C4 shape
//   accept_draws_check validate                 checks every validation branch; prints "validate ok"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ssa_accept_draws.hpp"

namespace ad = ecdna::accept_draws;

static int print_plan(int argc, char** argv) {
    if (argc < 5) return 2;
    const uint32_t keep = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const bool timepoints = std::strtoul(argv[3], nullptr, 10) != 0;
    const uint64_t mask = std::strtoull(argv[4], nullptr, 16);
    std::vector<uint32_t> m;
    for (int i = 5; i < argc; ++i) m.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    const ad::Plan p = ad::plan(9u, keep, timepoints, (uint32_t)m.size(), m.data(), mask);
    std::printf("slices %u mask %llx groups %u max_mp %u\n", p.n_slices, (unsigned long long)p.slice_mask, p.n_groups,
                p.max_mp);
    for (uint32_t s = 0; s < p.n_slices; ++s) std::printf("slice %u groups %u %u\n", s, p.slice_group[s], p.slice_group[s + 1]);
    for (uint32_t g = 0; g < p.n_groups; ++g) {
        std::printf("m %u targets", p.group_m[g]);
        for (uint32_t i = p.group_offset[g]; i < p.group_offset[g + 1]; ++i) std::printf(" %u", p.group_targets[i]);
        std::printf("\n");
    }
    return 0;
}

static int check_lds() {
    const uint32_t bins_list[] = {2, 9, 64, 65, 130, 1024, 2047, 2048};
    const uint32_t keep_list[] = {1, 2, 64, 199, 200, 2048, 4095, 4096};
    for (uint32_t bins : bins_list)
        for (uint32_t keep : keep_list)
            for (int timepoints = 0; timepoints < 2; ++timepoints) {
                std::vector<uint32_t> sizes(std::min(keep, 64u));
                for (uint32_t i = 0; i < sizes.size(); ++i) sizes[i] = keep / 2u > i ? keep / 2u - i : 1u;
                const ad::Plan p = ad::plan(bins, keep, timepoints != 0, (uint32_t)sizes.size(), sizes.data(), 0);
                if (p.max_mp != keep / 2u && !(keep == 1u && p.max_mp == 0u))
                    return std::fprintf(stderr, "max_mp %u at keep = %u\n", p.max_mp, keep), 1;
                const ecdna::thin::LdsPlan want = ecdna::thin::lds_plan(bins, p.max_mp);
                if (p.lds.waves != want.waves || p.lds.table_slots != want.table_slots ||
                    p.lds.scratch_words != want.scratch_words || p.lds.lds_bytes != want.lds_bytes)
                    return std::fprintf(stderr, "not the thinning pass's plan\n"), 1;
                if (p.lds.lds_bytes > ecdna::kPassLdsMax)
                    return std::fprintf(stderr, "%zu bytes at bins = %u, keep = %u\n", p.lds.lds_bytes, bins, keep), 1;
                if (p.lds.lds_bytes != p.lds.waves * (2u * (size_t)bins + p.lds.scratch_words) * 4u)
                    return std::fprintf(stderr, "lds_bytes\n"), 1;
            }
    const uint32_t half = 2048;
    const ad::Plan top = ad::plan(2048, 4096, false, 1u, &half, 0);
    std::printf("lds ok\nlimits max_mp %u waves %u table_slots %u scratch_words %u lds_bytes %zu\n", top.max_mp,
                top.lds.waves, top.lds.table_slots, top.lds.scratch_words, top.lds.lds_bytes);
    return 0;
}

static int print_bytes() {
    const uint64_t n = 4194304;  // the C4 sweep
    std::printf("passes %llu sums %llu cdf %llu scalars %llu loop %llu\n", (unsigned long long)ad::passes_bytes(n, 8),
                (unsigned long long)ad::sums_bytes(8, 1024), (unsigned long long)ad::cdf_bytes(2, 1025),
                (unsigned long long)ad::scalars_bytes(2), (unsigned long long)ad::loop_record_bytes(n, 64));
    return 0;
}

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

static int check_validate() {
    constexpr uint32_t bins = 5, P = 64, keep = 200;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<uint64_t> hists((size_t)P * bins, 1);
    std::vector<uint32_t> cells(P, keep);
    cells[3] = 1;
    std::vector<ecdna_accept_threshold_t> thr(32, ecdna_accept_threshold_t{0.5, inf, 0.0, 1.0});
    ecdna_ssa_accept_draws_t good{};
    good.struct_size = sizeof good;
    good.n_targets = P;
    good.target_hists = hists.data();
    good.sample_cells = cells.data();
    good.first_draw = 0;
    good.n_draws = 64;
    good.n_thresholds = 32;
    good.thresholds = thr.data();
    good.timepoint_mask = ~0ull;
    auto inv = [&](const ecdna_ssa_accept_draws_t& a, uint32_t T = 0, uint64_t n = 1000) {
        return ad::invalid(bins, keep, T, n, a);
    };
    int bad = 0;
    bad += expect(inv(good), nullptr, "a good block");
    ecdna_ssa_accept_draws_t a = good;
    a.timepoints = 1;
    bad += expect(inv(a, P), nullptr, "the timepoint store, T = P");
    bad += expect(inv(a, 0), nullptr, "the timepoint store on a context without it: its state decides");
    bad += expect(inv(a, 3), "n_targets must be T = 3", "n_targets != T");
    a = good;
    a.n_targets = 1;
    a.timepoint_mask = 1;
    a.first_draw = 63;
    a.n_draws = 1;
    a.n_thresholds = 1;
    bad += expect(inv(a), nullptr, "the smallest call");
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        a = good;
        a.struct_size = size;
        bad += expect(inv(a), "struct_size", "struct_size");
    }
    a = good;
    a.reserved = 1ull << 40;
    bad += expect(inv(a), "reserved", "reserved");
    for (uint32_t t : {2u, 0xffffffffu}) {
        a = good;
        a.timepoints = t;
        bad += expect(inv(a), "accept_draws.timepoints", "timepoints above 1");
    }
    for (uint32_t n : {0u, 65u, 0xffffffffu}) {
        a = good;
        a.n_targets = n;
        bad += expect(inv(a), "n_targets", "n_targets");
    }
    a = good;
    a.target_hists = nullptr;
    bad += expect(inv(a), "target_hists is NULL", "NULL target_hists");
    std::vector<uint64_t> holed = hists;
    for (uint32_t b = 0; b < bins; ++b) holed[(size_t)63 * bins + b] = 0;
    a = good;
    a.target_hists = holed.data();
    bad += expect(inv(a), "target_hists[63] is empty", "an all-zero row");
    holed[(size_t)63 * bins + bins - 1] = 1;  // mass in the overflow bin alone is a target
    bad += expect(inv(a), nullptr, "mass only in the last bin");
    a = good;
    a.sample_cells = nullptr;
    bad += expect(inv(a), "sample_cells is NULL", "NULL sample_cells");
    for (uint32_t m : {0u, keep + 1u, 4097u, 0xffffffffu}) {
        std::vector<uint32_t> cc = cells;
        cc[17] = m;
        a = good;
        a.sample_cells = cc.data();
        bad += expect(inv(a), "sample_cells[17]", "a size out of range");
        bad += expect(inv(a), "keep_cells = 200", "a size out of range names keep_cells");
    }
    for (uint32_t d : {0u, 65u, 0xffffffffu}) {
        a = good;
        a.n_draws = d;
        bad += expect(inv(a), "n_draws", "n_draws");
    }
    const uint32_t ranges[][2] = {{1, 64}, {64, 1}, {63, 2}, {0xffffffffu, 1}, {0xffffffffu, 2}, {32, 33}};
    for (const auto& r : ranges) {
        a = good;
        a.first_draw = r[0];
        a.n_draws = r[1];
        bad += expect(inv(a), "first_draw + n_draws", "a range past draw 63");
    }
    a = good;
    a.first_draw = 32;
    a.n_draws = 32;
    bad += expect(inv(a), nullptr, "the upper half of the draws");
    for (uint32_t q : {0u, 33u, 0xffffffffu}) {
        a = good;
        a.n_thresholds = q;
        bad += expect(inv(a), "n_thresholds", "n_thresholds");
    }
    a = good;
    a.thresholds = nullptr;
    bad += expect(inv(a), "thresholds is NULL", "NULL thresholds");
    const char* names[4] = {"thresholds[31].ks", "thresholds[31].mean_rel", "thresholds[31].entropy_rel",
                            "thresholds[31].frequency_diff"};
    for (int k = 0; k < 4; ++k)
        for (double v : {-1e-300, -inf, std::nan("")}) {
            std::vector<ecdna_accept_threshold_t> tt = thr;
            double* f[4] = {&tt[31].ks, &tt[31].mean_rel, &tt[31].entropy_rel, &tt[31].frequency_diff};
            *f[k] = v;
            a = good;
            a.thresholds = tt.data();
            bad += expect(inv(a), names[k], "a negative or NaN threshold");
        }
    a = good;
    a.n_targets = 3;
    a.timepoint_mask = 0b1000;
    bad += expect(inv(a), "timepoint_mask has bits at or above T = 3", "mask bits at T");
    a.timepoint_mask = 0b111;
    bad += expect(inv(a), nullptr, "every bit below T");
    a.timepoint_mask = 0;
    bad += expect(inv(a), nullptr, "mask 0: all");
    bad += expect(inv(good, 0, 1ull << 32), "n_replicates", "2^32 replicates");
    bad += expect(inv(good, 0, (1ull << 32) - 1), nullptr, "2^32 - 1 replicates");
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0) return print_plan(argc, argv);
    if (argc > 1 && std::strcmp(argv[1], "lds") == 0) return check_lds();
    if (argc > 1 && std::strcmp(argv[1], "bytes") == 0) return print_bytes();
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    std::fprintf(stderr, "usage: accept_draws_check plan K S MASK m0 m1 ... | lds | bytes | validate\n");
    return 2;
}
