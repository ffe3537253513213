// cohort_check.cpp — the host side of the cohort block (ecdna-evo_amd/csrc/ssa_cohort.hpp) on the CPU, for
// tests/test_cohort_native.py: the grouping of the targets by sample size, the LDS plan of the cohort pass and every
// branch of the block's validation. Built for the host alone, with the address and undefined-behaviour sanitizers.
//
//   cohort_check groups m0 m1 ...   prints the grouping of those sample sizes: "groups G max M", then per group
//                                   "m <size> targets t t ..."
//   cohort_check lds                checks the LDS plan over bins x bag_k x m, the limits included; prints "lds ok" and
//                                   the plan at the limits
//   cohort_check validate           checks every validation branch; prints "validate ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ssa_cohort.hpp"

namespace co = ecdna::cohort;

static int print_groups(int argc, char** argv) {
    std::vector<uint32_t> m;
    for (int i = 2; i < argc; ++i) m.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    const co::Groups g = co::group_by_sample_size(m.empty() ? nullptr : m.data(), (uint32_t)m.size());
    std::printf("groups %u max %u\n", g.n_groups, g.max_m);
    for (uint32_t j = 0; j < g.n_groups; ++j) {
        std::printf("m %u targets", g.m[j]);
        for (uint32_t i = g.offset[j]; i < g.offset[j + 1]; ++i) std::printf(" %u", g.targets[i]);
        std::printf("\n");
    }
    return 0;
}

static int check_lds() {
    const uint32_t bins_list[] = {2, 3, 17, 64, 65, 128, 257, 1024, 2047, 2048};
    const uint32_t bag_list[] = {0, 32, 64, 256};
    const uint32_t m_list[] = {0, 1, 2, 63, 64, 65, 300, 2048, 2049, 4095, 4096};
    for (uint32_t bins : bins_list)
        for (uint32_t bag_k : bag_list)
            for (uint32_t m : m_list) {
                const co::LdsPlan l = co::lds_plan(bins, bag_k, m);
                const uint32_t slots = m ? ecdna::subsample_table_slots(m) : 0u;
                if (l.table_slots != slots) return std::fprintf(stderr, "table_slots at m = %u\n", m), 1;
                if (m && (slots < 2u * m || (slots & (slots - 1u)))) return std::fprintf(stderr, "slots\n"), 1;
                // the scratch holds the table and, at other times, one f64 per bin
                if (l.scratch_words < slots || l.scratch_words < 2u * bins || (l.scratch_words & 1u))
                    return std::fprintf(stderr, "scratch at bins = %u, m = %u\n", bins, m), 1;
                const size_t per_wave = (2u * (size_t)bins + bag_k + l.scratch_words) * 4u;
                if (per_wave % 8u) return std::fprintf(stderr, "a wave's LDS is not 8-byte aligned\n"), 1;
                if (l.waves != 1u && l.waves != 2u && l.waves != 4u) return std::fprintf(stderr, "waves\n"), 1;
                if (l.lds_bytes != l.waves * per_wave) return std::fprintf(stderr, "lds_bytes\n"), 1;
                if (l.lds_bytes > ecdna::kPassLdsMax)
                    return std::fprintf(stderr, "%zu bytes at bins = %u, K = %u, m = %u\n", l.lds_bytes, bins, bag_k, m), 1;
                // as many waves as fit
                if (l.waves < 4u && 2u * l.waves * per_wave <= ecdna::kPassLdsMax)
                    return std::fprintf(stderr, "fewer waves than fit\n"), 1;
            }
    const co::LdsPlan top = co::lds_plan(2048, 256, 4096);
    std::printf("lds ok\nlimits waves %u table_slots %u scratch_words %u lds_bytes %zu\n", top.waves, top.table_slots,
                top.scratch_words, top.lds_bytes);
    return 0;
}

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

static int check_validate() {
    constexpr uint32_t bins = 5, P = 64;
    std::vector<uint64_t> hists((size_t)P * bins, 1);
    std::vector<uint32_t> cells(P, 4096);
    cells[3] = 1;
    ecdna_ssa_params_t p{};
    p.hist_bins = bins;
    p.flags = ECDNA_FLAG_REP_STATS;
    ecdna_ssa_cohort_t good{};
    good.struct_size = sizeof good;
    good.n_targets = P;
    good.target_hists = hists.data();
    good.sample_cells = cells.data();
    ecdna_ssa_ext_t ext{};
    ext.struct_size = sizeof ext;
    ecdna_ssa_passages_t pas{};
    int bad = 0;
    bad += expect(co::invalid(p, nullptr, nullptr, good), nullptr, "a good block");
    bad += expect(co::invalid(p, &ext, nullptr, good), nullptr, "a good block beside an idle extension block");
    ecdna_ssa_cohort_t c = good;
    c.sample_cells = nullptr;
    bad += expect(co::invalid(p, nullptr, nullptr, c), nullptr, "no samples");
    c = good;
    c.n_targets = 1;
    bad += expect(co::invalid(p, nullptr, nullptr, c), nullptr, "one target");
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        c = good;
        c.struct_size = size;
        bad += expect(co::invalid(p, nullptr, nullptr, c), "struct_size", "struct_size");
    }
    c = good;
    c.reserved = 1ull << 40;
    bad += expect(co::invalid(p, nullptr, nullptr, c), "reserved", "reserved");
    for (uint32_t n : {0u, 65u, 0xffffffffu}) {
        c = good;
        c.n_targets = n;
        bad += expect(co::invalid(p, nullptr, nullptr, c), "n_targets", "n_targets");
    }
    c = good;
    c.target_hists = nullptr;
    bad += expect(co::invalid(p, nullptr, nullptr, c), "target_hists is NULL", "NULL target_hists");
    ecdna_ssa_params_t q = p;
    q.flags = 0;
    bad += expect(co::invalid(q, nullptr, nullptr, good), "REP_STATS", "flags");
    bad += expect(co::invalid(p, nullptr, &pas, good), "passages", "a passage block");
    bad += expect(co::invalid(p, nullptr, &pas, good), "longitudinal", "a passage block");
    ext.snapshot_stats = 1;
    bad += expect(co::invalid(p, &ext, nullptr, good), "snapshot_stats", "snapshot statistics");
    bad += expect(co::invalid(p, &ext, nullptr, good), "longitudinal", "snapshot statistics");
    std::vector<uint64_t> holed = hists;
    for (uint32_t b = 0; b < bins; ++b) holed[(size_t)63 * bins + b] = 0;
    c = good;
    c.target_hists = holed.data();
    bad += expect(co::invalid(p, nullptr, nullptr, c), "target_hists[63] is empty", "an all-zero row");
    holed[(size_t)63 * bins + bins - 1] = 1;  // mass in the overflow bin alone is a target
    bad += expect(co::invalid(p, nullptr, nullptr, c), nullptr, "mass only in the last bin");
    for (uint32_t m : {0u, 4097u, 0xffffffffu}) {
        std::vector<uint32_t> cc = cells;
        cc[17] = m;
        c = good;
        c.sample_cells = cc.data();
        bad += expect(co::invalid(p, nullptr, nullptr, c), "sample_cells[17]", "a sample size out of range");
    }
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "groups") == 0) return print_groups(argc, argv);
    if (argc > 1 && std::strcmp(argv[1], "lds") == 0) return check_lds();
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    std::fprintf(stderr, "usage: cohort_check groups m0 m1 ... | lds | validate\n");
    return 2;
}
