// pool_draws_check.cpp — the host side of the pooling over thinning draws (ecdna-evo_amd/csrc/ssa_pool_draws.hpp) on
// the CPU, for tests/test_pool_draws_native.py: every branch of the call's validation, the verdict's and the pooling's
// grouping of the targets, the LDS plan at the limits, the byte counts and the launch-time check of the group tables the
// kernels index by. Built for the host alone, with the address and undefined-behaviour sanitizers.
//
//   pool_draws_check plan K S MASK m0 m1 ...  prints both groupings at keep_cells = K for store S (0 keep, 1 timepoints)
//                                             and timepoint mask MASK (hex): per grouping "verdict|pool slices N mask M
//                                             groups G max_mp X", then per slice "slice s groups a b", per group
//                                             "m <size> targets t t ..."; then "lds max_mp X"
//   pool_draws_check lds                      checks the plan's LDS over bins x keep_cells; prints "lds ok" and the plan
//                                             at bins 2 and 2048 with keep_cells 1 and 4096
//   pool_draws_check bytes                    prints the byte counts of two shapes
//   pool_draws_check validate                 checks every validation branch; prints "validate ok"
//   pool_draws_check grouping                 grouping_ok (ssa_launch.h), the launches' check of the group tables: prints
//                                             "accepted N" for the N groupings the two plans make over the sweep of
//                                             `lds` and three masks, then "refused <what>" per hand-broken table
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ssa_pool_draws.hpp"

namespace ad = ecdna::accept_draws;
namespace pd = ecdna::pool_draws;

static void print_grouping(const char* name, const ad::Plan& p) {
    std::printf("%s slices %u mask %llx groups %u max_mp %u\n", name, p.n_slices, (unsigned long long)p.slice_mask,
                p.n_groups, p.max_mp);
    for (uint32_t s = 0; s < p.n_slices; ++s)
        std::printf("slice %u groups %u %u\n", s, p.slice_group[s], p.slice_group[s + 1]);
    for (uint32_t g = 0; g < p.n_groups; ++g) {
        std::printf("m %u targets", p.group_m[g]);
        for (uint32_t i = p.group_offset[g]; i < p.group_offset[g + 1]; ++i) std::printf(" %u", p.group_targets[i]);
        std::printf("\n");
    }
}

static int print_plan(int argc, char** argv) {
    if (argc < 5) return 2;
    const uint32_t keep = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const bool timepoints = std::strtoul(argv[3], nullptr, 10) != 0;
    const uint64_t mask = std::strtoull(argv[4], nullptr, 16);
    std::vector<uint32_t> m;
    for (int i = 5; i < argc; ++i) m.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    const pd::Plan p = pd::plan(9u, keep, timepoints, (uint32_t)m.size(), m.data(), mask);
    print_grouping("verdict", p.verdict);
    print_grouping("pool", p.pool);
    const ecdna::thin::LdsPlan want = pd::lds_plan(9u, p.pool.max_mp);
    if (p.lds.waves != want.waves || p.lds.table_slots != want.table_slots || p.lds.scratch_words != want.scratch_words ||
        p.lds.lds_bytes != want.lds_bytes)
        return std::fprintf(stderr, "the plan's LDS is not the pooling grouping's\n"), 1;
    std::printf("lds max_mp %u\n", p.pool.max_mp);
    return 0;
}

// thin's per-wave plan, grown by the words of the accumulator ([bins] u32, evened) that do not fit behind the table
static size_t wave_bytes(uint32_t bins, uint32_t table_slots, uint32_t scratch_words) {
    const size_t need = (size_t)table_slots + bins + (bins & 1u);
    return (2u * (size_t)bins + (need > scratch_words ? need : (size_t)scratch_words)) * 4u;
}

static int check_lds() {
    const uint32_t bins_list[] = {2, 9, 64, 65, 130, 1024, 2047, 2048};
    const uint32_t keep_list[] = {1, 2, 64, 199, 200, 2048, 4095, 4096};
    for (uint32_t bins : bins_list)
        for (uint32_t keep : keep_list)
            for (int timepoints = 0; timepoints < 2; ++timepoints) {
                std::vector<uint32_t> sizes(std::min(keep, 64u));
                for (uint32_t i = 0; i < sizes.size(); ++i) sizes[i] = keep / 2u > i ? keep / 2u - i : 1u;
                // the mask leaves target 0, the largest m', out of the verdict: the pooling grouping still sizes the table
                const uint64_t mask = sizes.size() > 1 ? 2ull : 0ull;
                const pd::Plan p = pd::plan(bins, keep, timepoints != 0, (uint32_t)sizes.size(), sizes.data(), mask);
                if (p.pool.max_mp != keep / 2u && !(keep == 1u && p.pool.max_mp == 0u))
                    return std::fprintf(stderr, "max_mp %u at keep = %u\n", p.pool.max_mp, keep), 1;
                if (p.verdict.max_mp > p.pool.max_mp) return std::fprintf(stderr, "the verdict picks more\n"), 1;
                const ecdna::thin::LdsPlan thin = ecdna::thin::lds_plan(bins, p.pool.max_mp);
                if (p.lds.table_slots != thin.table_slots || p.lds.scratch_words != thin.scratch_words)
                    return std::fprintf(stderr, "not the thinning pass's table\n"), 1;
                if (p.lds.waves != 1u && p.lds.waves != 2u && p.lds.waves != 4u) return std::fprintf(stderr, "waves\n"), 1;
                if (p.lds.lds_bytes > ecdna::kPassLdsMax)
                    return std::fprintf(stderr, "%zu bytes at bins = %u, keep = %u\n", p.lds.lds_bytes, bins, keep), 1;
                const size_t per_wave = wave_bytes(bins, p.lds.table_slots, p.lds.scratch_words);
                if (p.lds.lds_bytes != p.lds.waves * per_wave ||
                    per_wave != (size_t)ecdna::pool_draws_wave_words(bins, p.lds.table_slots) * 4u)
                    return std::fprintf(stderr, "lds_bytes\n"), 1;
                // never below thin's plan nor above it plus one [bins] u32 array; room for the table and the
                // accumulator side by side behind the two histograms; every wave's scratch 8-byte aligned
                const size_t thin_wave = thin.lds_bytes / thin.waves;
                if (per_wave < thin_wave || per_wave > thin_wave + ((size_t)bins + 1u) * 4u || per_wave % 8u ||
                    per_wave < (2u * (size_t)bins + p.lds.table_slots + bins) * 4u)
                    return std::fprintf(stderr, "per wave %zu bytes at bins = %u\n", per_wave, bins), 1;
                // as many waves as fit: twice as many would not
                if (p.lds.waves < 4u && 2u * p.lds.waves * per_wave <= ecdna::kPassLdsMax)
                    return std::fprintf(stderr, "more waves fit at bins = %u, keep = %u\n", bins, keep), 1;
            }
    std::puts("lds ok");
    for (uint32_t bins : {2u, 2048u})
        for (uint32_t keep : {1u, 4096u}) {
            const uint32_t half = keep > 1u ? keep / 2u : 1u;
            const pd::Plan p = pd::plan(bins, keep, false, 1u, &half, 0);
            std::printf("bins %u keep %u max_mp %u waves %u table_slots %u scratch_words %u lds_bytes %zu\n", bins, keep,
                        p.pool.max_mp, p.lds.waves, p.lds.table_slots, p.lds.scratch_words, p.lds.lds_bytes);
        }
    return 0;
}

static int print_bytes() {
    // two biopsies on the keep store of the C4 sweep's sets; four timepoints
    std::printf("thinned %llu kept %llu pooled %llu cdf %llu scalars %llu\n",
                (unsigned long long)pd::thinned_words(2, 1024, 1025), (unsigned long long)pd::kept_words(1, 1024, 1025),
                (unsigned long long)pd::pooled_bytes(2, 1, 1024, 1025), (unsigned long long)pd::cdf_bytes(2, 1025),
                (unsigned long long)pd::scalars_bytes(2));
    std::printf("thinned %llu kept %llu pooled %llu cdf %llu scalars %llu\n",
                (unsigned long long)pd::thinned_words(4, 3, 33), (unsigned long long)pd::kept_words(4, 3, 33),
                (unsigned long long)pd::pooled_bytes(4, 4, 3, 33), (unsigned long long)pd::cdf_bytes(4, 33),
                (unsigned long long)pd::scalars_bytes(4));
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
    uint64_t out = 0;  // (the outputs are only tested against NULL)
    auto inv = [&](const ecdna_ssa_accept_draws_t& a, uint32_t q = 0, const void* thinned = nullptr,
                   const void* kept = nullptr, uint32_t T = 0, uint64_t n = 1000) {
        return pd::invalid(bins, keep, T, n, a, q, thinned, kept);
    };
    // whatever accept_draws::invalid says of the block, this call says, word for word, whatever its own arguments
    auto same = [&](const ecdna_ssa_accept_draws_t& a, const char* word, const char* what, uint32_t T = 0,
                    uint64_t n = 1000) {
        const std::string want = ad::invalid(bins, keep, T, n, a);
        int bad = expect(want, word, what);
        if (inv(a, 0, &out, &out, T, n) != want || (word && inv(a, 0xffffffffu, nullptr, nullptr, T, n) != want))
            bad += std::fprintf(stderr, "%s: not accept_draws' message\n", what), 1;
        return bad;
    };
    int bad = 0;
    bad += expect(inv(good, 0, &out, &out), nullptr, "a good call");
    bad += expect(inv(good, 31, &out, nullptr), nullptr, "the last row, thinned alone");
    bad += expect(inv(good, 31, nullptr, &out), nullptr, "the last row, kept alone");
    // the call's own arguments
    for (uint32_t q : {32u, 33u, 0xffffffffu})
        bad += expect(inv(good, q, &out, &out), "pool_draws.threshold must be < accept_draws.n_thresholds = 32",
                      "threshold >= Q");
    ecdna_ssa_accept_draws_t a = good;
    a.n_thresholds = 1;
    bad += expect(inv(a, 0, &out, &out), nullptr, "one row");
    bad += expect(inv(a, 1, &out, &out), "n_thresholds = 1", "threshold 1 of one row");
    bad += expect(inv(good, 0, nullptr, nullptr), "pool_draws.out_thinned and pool_draws.out_kept are both NULL",
                  "both outputs NULL");
    bad += expect(inv(good, 32, nullptr, nullptr), "pool_draws.threshold", "the threshold is named before the outputs");
    // everything accept_draws refuses, with the same messages
    a = good;
    a.timepoints = 1;
    bad += same(a, nullptr, "the timepoint store, T = P", P);
    bad += same(a, nullptr, "the timepoint store on a context without it: its state decides", 0);
    bad += same(a, "n_targets must be T = 3", "n_targets != T", 3);
    for (uint32_t size : {0u, (uint32_t)sizeof good - 4u, (uint32_t)sizeof good + 8u}) {
        a = good;
        a.struct_size = size;
        bad += same(a, "accept_draws.struct_size", "struct_size");
    }
    a = good;
    a.reserved = 1ull << 40;
    bad += same(a, "accept_draws.reserved", "reserved");
    for (uint32_t t : {2u, 0xffffffffu}) {
        a = good;
        a.timepoints = t;
        bad += same(a, "accept_draws.timepoints", "timepoints above 1");
    }
    for (uint32_t n : {0u, 65u, 0xffffffffu}) {
        a = good;
        a.n_targets = n;
        bad += same(a, "accept_draws.n_targets", "n_targets");
    }
    a = good;
    a.target_hists = nullptr;
    bad += same(a, "target_hists is NULL", "NULL target_hists");
    std::vector<uint64_t> holed = hists;
    for (uint32_t b = 0; b < bins; ++b) holed[(size_t)63 * bins + b] = 0;
    a = good;
    a.target_hists = holed.data();
    bad += same(a, "target_hists[63] is empty", "an all-zero row");
    a = good;
    a.sample_cells = nullptr;
    bad += same(a, "sample_cells is NULL", "NULL sample_cells");
    for (uint32_t m : {0u, keep + 1u, 0xffffffffu}) {
        std::vector<uint32_t> cc = cells;
        cc[17] = m;
        a = good;
        a.sample_cells = cc.data();
        bad += same(a, "sample_cells[17]", "a size out of range");
    }
    for (uint32_t d : {0u, 65u}) {
        a = good;
        a.n_draws = d;
        bad += same(a, "accept_draws.n_draws", "n_draws");
    }
    a = good;
    a.first_draw = 63;
    a.n_draws = 2;
    bad += same(a, "first_draw + n_draws", "a range past draw 63");
    for (uint32_t q : {0u, 33u}) {
        a = good;
        a.n_thresholds = q;
        bad += same(a, "accept_draws.n_thresholds", "n_thresholds");
    }
    a = good;
    a.thresholds = nullptr;
    bad += same(a, "thresholds is NULL", "NULL thresholds");
    for (double v : {-1e-300, std::nan("")}) {
        std::vector<ecdna_accept_threshold_t> tt = thr;
        tt[31].entropy_rel = v;
        a = good;
        a.thresholds = tt.data();
        bad += same(a, "thresholds[31].entropy_rel", "a negative or NaN threshold");
    }
    a = good;
    a.n_targets = 3;
    a.timepoint_mask = 0b1000;
    bad += same(a, "timepoint_mask has bits at or above T = 3", "mask bits at T");
    bad += same(good, "n_replicates", "2^32 replicates", 0, 1ull << 32);
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

// grouping_ok takes what accept_draws::plan and pool_draws::plan make and refuses a table broken in any one way: one
// refusal per clause of the check, each on a grouping that is in order otherwise.
static int check_grouping() {
    const uint32_t bins_list[] = {2, 9, 64, 65, 130, 1024, 2047, 2048};
    const uint32_t keep_list[] = {1, 2, 64, 199, 200, 2048, 4095, 4096};
    unsigned accepted = 0;
    for (uint32_t bins : bins_list)
        for (uint32_t keep : keep_list)
            for (int timepoints = 0; timepoints < 2; ++timepoints) {
                std::vector<uint32_t> sizes(std::min(keep, 64u));
                for (uint32_t i = 0; i < sizes.size(); ++i) sizes[i] = keep / 2u > i ? keep / 2u - i : 1u;
                const uint32_t P = (uint32_t)sizes.size();
                const uint64_t all = P >= 64u ? ~0ull : (1ull << P) - 1ull;
                for (uint64_t mask : {0ull, P > 1u ? 2ull : 0ull, 0x5555555555555555ull & all}) {
                    const pd::Plan p = pd::plan(bins, keep, timepoints != 0, P, sizes.data(), mask);
                    const ad::Plan v = ad::plan(bins, keep, timepoints != 0, P, sizes.data(), mask);
                    if (std::memcmp(&v.grouping(), &p.verdict.grouping(), sizeof(ecdna::Grouping)) != 0)
                        return std::fprintf(stderr, "the verdict's grouping is not accept_draws'\n"), 1;
                    for (const ad::Plan* q : {&p.verdict, &p.pool, &v}) {
                        if (!ecdna::grouping_ok(*q, q->n_slices, P, keep))
                            return std::fprintf(stderr, "a plan's grouping refused at bins = %u, keep = %u, store %d, "
                                                        "mask %llx\n", bins, keep, timepoints, (unsigned long long)mask), 1;
                        ++accepted;
                    }
                }
            }
    std::printf("accepted %u\n", accepted);

    // the keep store, four targets of two sizes: groups (100: 0 2) (80: 1 3); the timepoint store, three slices
    const uint32_t keep_sizes[] = {100, 80, 100, 80}, tp_sizes[] = {20, 50, 35};
    const ecdna::Grouping keep = ad::plan(9u, 200u, false, 4u, keep_sizes, 0);
    const ecdna::Grouping tp = ad::plan(9u, 50u, true, 3u, tp_sizes, 0);
    if (!ecdna::grouping_ok(keep, 1u, 4u, 200u) || !ecdna::grouping_ok(tp, 3u, 3u, 50u) || keep.n_groups != 2u ||
        tp.n_groups != 3u)
        return std::fprintf(stderr, "the groupings to break are not in order\n"), 1;
    int bad = 0;
    auto refused = [&](const ecdna::Grouping& g, uint32_t n_slices, uint32_t n_targets, uint32_t m, const char* what) {
        if (ecdna::grouping_ok(g, n_slices, n_targets, m))
            bad += std::fprintf(stderr, "taken: %s\n", what), 1;
        else
            std::printf("refused %s\n", what);
    };
    ecdna::Grouping g = keep;
    g.group_offset[1] = 5;  // 0 5 4
    refused(g, 1, 4, 200, "a decreasing group_offset");
    g = tp;
    g.slice_group[1] = 3;  // 0 3 2 3
    refused(g, 3, 3, 50, "a decreasing slice_group");
    g = keep;
    g.slice_group[1] = 1;
    refused(g, 1, 4, 200, "slice_group[n_slices] != n_groups");
    g = keep;
    g.group_targets[3] = 4;
    refused(g, 1, 4, 200, "a target index >= n_targets");
    g = keep;
    g.group_m[1] = 0;
    refused(g, 1, 4, 200, "group_m of 0");
    g = keep;
    g.group_m[1] = 201;
    refused(g, 1, 4, 200, "group_m of m + 1");
    g = keep;
    g.n_groups = 0;
    g.slice_group[1] = 0;
    refused(g, 1, 4, 200, "n_groups of 0");
    g = keep;
    g.n_groups = 5;  // five groups over four targets: the last three empty, every table in order otherwise
    g.slice_group[1] = 5;
    for (uint32_t j = 2; j < 5; ++j) g.group_m[j] = 1, g.group_offset[j + 1] = 4;
    refused(g, 1, 4, 200, "n_groups of n_targets + 1");
    g = keep;
    g.slice_group[0] = 1;
    refused(g, 1, 4, 200, "slice_group[0] != 0");
    g = keep;
    g.group_offset[0] = 1;
    refused(g, 1, 4, 200, "group_offset[0] != 0");
    g = keep;
    g.group_offset[2] = 5;
    refused(g, 1, 4, 200, "group_offset[n_groups] > n_targets");
    refused(keep, 0, 4, 200, "no slice");
    refused(keep, 65, 4, 200, "65 slices");
    refused(keep, 1, 65, 200, "65 targets");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0) return print_plan(argc, argv);
    if (argc > 1 && std::strcmp(argv[1], "lds") == 0) return check_lds();
    if (argc > 1 && std::strcmp(argv[1], "bytes") == 0) return print_bytes();
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    if (argc > 1 && std::strcmp(argv[1], "grouping") == 0) return check_grouping();
    std::fprintf(stderr, "usage: pool_draws_check plan K S MASK m0 m1 ... | lds | bytes | validate | grouping\n");
    return 2;
}
