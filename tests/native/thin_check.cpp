// thin_check.cpp — the host side of the sized rescore (ecdna-evo_amd/csrc/ssa_thin.hpp) on the CPU, for
// tests/test_thin_native.py: the grouping of the targets by (measured cells, draw index), the thinning stream's tag, the
// LDS plan of the thinning pass and every branch of the two calls' validation. Built for the host alone, with the
// address and undefined-behaviour sanitizers.
//
//   thin_check groups K m0:d0 m1:d1 ...  prints the grouping at keep_cells = K: "groups G max_mp M", then per group
//                                        "m <size> d <draw> targets t t ..."
//   thin_check tag                       checks the tag's fields; prints "tag ok" and the tag at s = 63, d = 63
//   thin_check lds                       checks the LDS plan over bins x keep_cells, the limits included; prints
//                                        "lds ok" and the plan at the limits
//   thin_check validate                  checks every validation branch; prints "validate ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ssa_thin.hpp"

namespace th = ecdna::thin;

static int print_groups(int argc, char** argv) {
    if (argc < 3) return 2;
    const uint32_t keep = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    std::vector<uint32_t> m, d;
    bool with_draws = false;
    for (int i = 3; i < argc; ++i) {
        char* end = nullptr;
        m.push_back((uint32_t)std::strtoul(argv[i], &end, 10));
        if (*end == ':') with_draws = true;
        d.push_back(*end == ':' ? (uint32_t)std::strtoul(end + 1, nullptr, 10) : 0u);
    }
    const th::Groups g = th::group_by_size_and_draw(m.empty() ? nullptr : m.data(), with_draws ? d.data() : nullptr,
                                                    (uint32_t)m.size(), keep);
    std::printf("groups %u max_mp %u\n", g.n_groups, g.max_mp);
    for (uint32_t j = 0; j < g.n_groups; ++j) {
        std::printf("m %u d %u targets", g.m[j], g.d[j]);
        for (uint32_t i = g.offset[j]; i < g.offset[j + 1]; ++i) std::printf(" %u", g.targets[i]);
        std::printf("\n");
    }
    return 0;
}

static int check_tag() {
    constexpr uint32_t kBlock = 0x3ffu, kDraw = 0x3fu << 10, kSnap = 0x7fu << 16, kFlag = 1u << 29, kTag = 3u << 30;
    static_assert((kBlock & kDraw) == 0 && (kDraw & kSnap) == 0 && (kSnap & kFlag) == 0 && (kFlag & kTag) == 0, "masks");
    for (uint32_t s1 = 0; s1 <= 64u; ++s1)      // snapshot_plus_one: 0 (the end of the run, a phase), s + 1 for s < 64
        for (uint32_t d = 0; d <= th::kMaxDraw; ++d) {
            const uint32_t tag = th::stream_tag(s1, d);
            if ((tag & kBlock) != 0u) return std::fprintf(stderr, "the block index's bits are taken\n"), 1;
            if ((tag & kDraw) != (d << 10)) return std::fprintf(stderr, "draw field at d = %u\n", d), 1;
            if ((tag & kSnap) != (s1 << 16)) return std::fprintf(stderr, "snapshot field at s + 1 = %u\n", s1), 1;
            if ((tag & kFlag) != kFlag || (tag & kTag) != kTag) return std::fprintf(stderr, "flag or tag\n"), 1;
            if (tag & ~(kBlock | kDraw | kSnap | kFlag | kTag)) return std::fprintf(stderr, "a stray bit\n"), 1;
            // with the thinning flag cleared it is the stream the slice's own sample was drawn on
            if ((tag & ~(kFlag | kDraw)) != (0xC0000000u | (s1 << 16))) return std::fprintf(stderr, "base tag\n"), 1;
        }
    // s = 63, d = 63, t = 1023: every field at its largest, still disjoint
    const uint32_t top = th::stream_tag(64u, 63u) | 1023u;
    if (top != (0xC0000000u | (64u << 16) | 0x20000000u | (63u << 10) | 1023u)) return std::fprintf(stderr, "top\n"), 1;
    if (__builtin_popcount(top) != 2 + 1 + 1 + 6 + 10) return std::fprintf(stderr, "fields meet at the top\n"), 1;
    std::printf("tag ok\ntop 0x%08x\n", top);
    return 0;
}

static int check_lds() {
    const uint32_t bins_list[] = {2, 3, 9, 33, 64, 65, 257, 1024, 2047, 2048};
    const uint32_t keep_list[] = {1, 2, 3, 64, 65, 199, 200, 2048, 4095, 4096};
    for (uint32_t bins : bins_list)
        for (uint32_t keep : keep_list) {
            // the largest m' over every m1 in 1 .. keep is keep / 2
            std::vector<uint32_t> all(std::min(keep, 64u));
            for (uint32_t i = 0; i < all.size(); ++i) all[i] = keep / 2u > i ? keep / 2u - i : 1u;
            const th::Groups g = th::group_by_size_and_draw(all.data(), nullptr, (uint32_t)all.size(), keep);
            if (g.max_mp != keep / 2u && !(keep == 1u && g.max_mp == 0u))
                return std::fprintf(stderr, "max_mp %u at keep = %u\n", g.max_mp, keep), 1;
            const th::LdsPlan l = th::lds_plan(bins, g.max_mp);
            const uint32_t slots = g.max_mp ? ecdna::subsample_table_slots(g.max_mp) : 0u;
            if (l.table_slots != slots) return std::fprintf(stderr, "table_slots\n"), 1;
            if (g.max_mp && (slots < 2u * g.max_mp || (slots & (slots - 1u)))) return std::fprintf(stderr, "slots\n"), 1;
            if (l.scratch_words < slots || l.scratch_words < 2u * bins || (l.scratch_words & 1u))
                return std::fprintf(stderr, "scratch at bins = %u, keep = %u\n", bins, keep), 1;
            const size_t per_wave = (2u * (size_t)bins + l.scratch_words) * 4u;
            if (per_wave % 8u) return std::fprintf(stderr, "a wave's LDS is not 8-byte aligned\n"), 1;
            if (l.waves != 1u && l.waves != 2u && l.waves != 4u) return std::fprintf(stderr, "waves\n"), 1;
            if (l.lds_bytes != l.waves * per_wave) return std::fprintf(stderr, "lds_bytes\n"), 1;
            if (l.lds_bytes > ecdna::kPassLdsMax)
                return std::fprintf(stderr, "%zu bytes at bins = %u, keep = %u\n", l.lds_bytes, bins, keep), 1;
            if (l.waves < 4u && 2u * l.waves * per_wave <= ecdna::kPassLdsMax)
                return std::fprintf(stderr, "fewer waves than fit\n"), 1;
        }
    const uint32_t half = 2048;
    const th::Groups g = th::group_by_size_and_draw(&half, nullptr, 1u, 4096u);
    const th::LdsPlan top = th::lds_plan(2048, g.max_mp);
    std::printf("lds ok\nlimits max_mp %u waves %u table_slots %u scratch_words %u lds_bytes %zu\n", g.max_mp, top.waves,
                top.table_slots, top.scratch_words, top.lds_bytes);
    return 0;
}

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

static int check_validate() {
    constexpr uint32_t bins = 5, P = 64, keep = 200;
    std::vector<uint64_t> hists((size_t)P * bins, 1);
    std::vector<uint32_t> cells(P, keep), draws(P, 63);
    cells[3] = 1;
    draws[5] = 0;
    ecdna_ssa_rescore_t good{};
    good.struct_size = sizeof good;
    good.n_targets = P;
    good.target_hists = hists.data();
    good.sample_cells = cells.data();
    good.sample_draws = draws.data();
    int bad = 0;
    bad += expect(th::invalid(bins, keep, good), nullptr, "a good block");
    ecdna_ssa_rescore_t r = good;
    r.sample_cells = nullptr;
    bad += expect(th::invalid(bins, keep, r), nullptr, "no sizes");
    r = good;
    r.sample_draws = nullptr;
    bad += expect(th::invalid(bins, keep, r), nullptr, "no draws");
    r = good;
    r.n_targets = 1;
    bad += expect(th::invalid(bins, keep, r), nullptr, "one target");
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        r = good;
        r.struct_size = size;
        bad += expect(th::invalid(bins, keep, r), "struct_size", "struct_size");
    }
    r = good;
    r.reserved = 1ull << 40;
    bad += expect(th::invalid(bins, keep, r), "reserved", "reserved");
    for (uint32_t n : {0u, 65u, 0xffffffffu}) {
        r = good;
        r.n_targets = n;
        bad += expect(th::invalid(bins, keep, r), "n_targets", "n_targets");
    }
    r = good;
    r.target_hists = nullptr;
    bad += expect(th::invalid(bins, keep, r), "target_hists is NULL", "NULL target_hists");
    std::vector<uint64_t> holed = hists;
    for (uint32_t b = 0; b < bins; ++b) holed[(size_t)63 * bins + b] = 0;
    r = good;
    r.target_hists = holed.data();
    bad += expect(th::invalid(bins, keep, r), "target_hists[63] is empty", "an all-zero row");
    holed[(size_t)63 * bins + bins - 1] = 1;  // mass in the overflow bin alone is a target
    bad += expect(th::invalid(bins, keep, r), nullptr, "mass only in the last bin");
    for (uint32_t m : {0u, keep + 1u, 4097u, 0xffffffffu}) {
        std::vector<uint32_t> cc = cells;
        cc[17] = m;
        r = good;
        r.sample_cells = cc.data();
        bad += expect(th::invalid(bins, keep, r), "sample_cells[17]", "a size out of range");
        bad += expect(th::invalid(bins, keep, r), "keep_cells = 200", "a size out of range names keep_cells");
    }
    for (uint32_t d : {64u, 0xffffffffu}) {
        std::vector<uint32_t> dd = draws;
        dd[9] = d;
        r = good;
        r.sample_draws = dd.data();
        bad += expect(th::invalid(bins, keep, r), "sample_draws[9]", "a draw out of range");
        r.sample_cells = nullptr;  // (ignored then, but still checked)
        bad += expect(th::invalid(bins, keep, r), "sample_draws[9]", "a draw out of range without sizes");
    }

    // the timepoint call: T = 3 targets, sizes or none, one draw
    constexpr uint32_t T = 3;
    const uint32_t tc[T] = {keep, 1, 70};
    bad += expect(th::invalid_timepoints(bins, keep, T, hists.data(), tc, 0), nullptr, "good timepoints");
    bad += expect(th::invalid_timepoints(bins, keep, T, hists.data(), nullptr, 63), nullptr, "no sizes, a draw");
    bad += expect(th::invalid_timepoints(bins, keep, T, nullptr, tc, 0), "target_hists is NULL", "NULL targets");
    std::vector<uint64_t> holed_t(hists.begin(), hists.begin() + (size_t)T * bins);
    for (uint32_t b = 0; b < bins; ++b) holed_t[(size_t)1 * bins + b] = 0;
    bad += expect(th::invalid_timepoints(bins, keep, T, holed_t.data(), tc, 0), "target_hists[1] is empty", "a hole");
    for (uint32_t m : {0u, keep + 1u}) {
        const uint32_t bc[T] = {keep, 1, m};
        bad += expect(th::invalid_timepoints(bins, keep, T, hists.data(), bc, 0), "sample_cells[2]", "a size");
    }
    bad += expect(th::invalid_timepoints(bins, keep, T, hists.data(), tc, 64), "draw", "the draw");
    bad += expect(th::invalid_timepoints(bins, keep, T, hists.data(), nullptr, 64), "draw", "the draw without sizes");
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "groups") == 0) return print_groups(argc, argv);
    if (argc > 1 && std::strcmp(argv[1], "tag") == 0) return check_tag();
    if (argc > 1 && std::strcmp(argv[1], "lds") == 0) return check_lds();
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    std::fprintf(stderr, "usage: thin_check groups K m0:d0 m1:d1 ... | tag | lds | validate\n");
    return 2;
}
