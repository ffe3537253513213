// select_draws_check.cpp — the host side of the select over thinning draws (ecdna-evo_amd/csrc/ssa_select_draws.hpp) on
// the CPU, for tests/test_select_draws_native.py: every branch of the call's validation with its message, that
// accept_draws::invalid answers as before, the byte counts with the 32-bit bound of the keys, and the comparison "same
// block as the cached keys". Built for the host alone, with the address and undefined-behaviour sanitizers.
//
//   select_draws_check validate   checks every validation branch; prints "validate ok"
//   select_draws_check bytes      prints the byte counts of three shapes and what the bound says of them
//   select_draws_check same       checks the same-block comparison; prints "same ok"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ssa_select_draws.hpp"

namespace ad = ecdna::accept_draws;
namespace sd = ecdna::select_draws;

static int expect(const std::string& got, const char* word, const char* what) {
    if (word ? got.find(word) == std::string::npos : !got.empty())
        return std::fprintf(stderr, "%s: got \"%s\"\n", what, got.c_str()), 1;
    return 0;
}

constexpr uint32_t kBins = 5, kP = 64, kKeep = 200;

// A block ecdna_ssa_ctx_accept_draws takes, and the arrays it points into.
struct Good {
    std::vector<uint64_t> hists = std::vector<uint64_t>((size_t)kP * kBins, 1);
    std::vector<uint32_t> cells = std::vector<uint32_t>(kP, kKeep);
    std::vector<ecdna_accept_threshold_t> thr = std::vector<ecdna_accept_threshold_t>(
        32, ecdna_accept_threshold_t{0.5, std::numeric_limits<double>::infinity(), 0.0, 1.0});
    ecdna_ssa_accept_draws_t with{}, without{};
    Good() {
        cells[3] = 1;
        with.struct_size = sizeof with;
        with.n_targets = kP;
        with.target_hists = hists.data();
        with.sample_cells = cells.data();
        with.first_draw = 0;
        with.n_draws = 64;
        with.n_thresholds = 32;
        with.thresholds = thr.data();
        with.timepoint_mask = ~0ull;
        without = with;
        without.n_thresholds = 0;
        without.thresholds = nullptr;
    }
};

static int check_validate() {
    const Good good;
    auto inv = [&](const ecdna_ssa_accept_draws_t& a, uint32_t T = 0, uint64_t n = 1000) {
        return sd::invalid(kBins, kKeep, T, n, a);
    };
    // whatever accept_draws::invalid says of the block with threshold rows, this call says of the block without them
    auto same = [&](ecdna_ssa_accept_draws_t a, const char* word, const char* what, uint32_t T = 0, uint64_t n = 1000) {
        const std::string got = inv(a, T, n);
        a.n_thresholds = 32;
        a.thresholds = good.thr.data();
        const std::string want = ad::invalid(kBins, kKeep, T, n, a);
        int bad = expect(want, word, what);
        if (got != want) bad += std::fprintf(stderr, "%s: \"%s\" is not accept_draws' message\n", what, got.c_str()), 1;
        if (ad::invalid(kBins, kKeep, T, n, a, false) != want)
            bad += std::fprintf(stderr, "%s: the parameter's default is not `false`\n", what), 1;
        return bad;
    };
    int bad = 0;
    // with and without threshold rows: each call takes its own block and refuses the other's
    bad += expect(ad::invalid(kBins, kKeep, 0, 1000, good.with), nullptr, "accept_draws takes its block");
    bad += expect(inv(good.without), nullptr, "select_draws takes the block without rows");
    bad += expect(inv(good.with), "select_draws.n_thresholds must be 0", "select_draws refuses threshold rows");
    bad += expect(ad::invalid(kBins, kKeep, 0, 1000, good.without), "accept_draws.n_thresholds must be in [1, 32]",
                  "accept_draws refuses the block without rows");
    ecdna_ssa_accept_draws_t a = good.without;
    a.thresholds = good.thr.data();
    bad += expect(inv(a), "select_draws.thresholds must be NULL", "rows without a count");
    bad += expect(ad::invalid(kBins, kKeep, 0, 1000, a), "accept_draws.n_thresholds", "accept_draws names the count first");
    a = good.without;
    a.n_thresholds = 1;
    bad += expect(inv(a), "select_draws.n_thresholds", "a count without rows");
    bad += expect(ad::invalid(kBins, kKeep, 0, 1000, a), "accept_draws.thresholds is NULL", "accept_draws: NULL rows");
    // accept_draws' own threshold rules are as they were
    for (uint32_t q : {0u, 33u}) {
        a = good.with;
        a.n_thresholds = q;
        bad += expect(ad::invalid(kBins, kKeep, 0, 1000, a), "accept_draws.n_thresholds must be in [1, 32]", "Q");
    }
    for (double v : {-1e-300, std::nan("")}) {
        std::vector<ecdna_accept_threshold_t> tt = good.thr;
        tt[31].entropy_rel = v;
        a = good.with;
        a.thresholds = tt.data();
        bad += expect(ad::invalid(kBins, kKeep, 0, 1000, a), "accept_draws.thresholds[31].entropy_rel must be >= 0",
                      "a negative or NaN threshold");
    }
    // everything else accept_draws refuses, with the same messages
    a = good.without;
    a.timepoints = 1;
    bad += same(a, nullptr, "the timepoint store, T = P", kP);
    bad += same(a, nullptr, "the timepoint store on a context without it: its state decides", 0);
    bad += same(a, "n_targets must be T = 3", "n_targets != T", 3);
    for (uint32_t size : {0u, (uint32_t)sizeof a - 4u, (uint32_t)sizeof a + 8u}) {
        a = good.without;
        a.struct_size = size;
        bad += same(a, "accept_draws.struct_size", "struct_size");
    }
    a = good.without;
    a.reserved = 1ull << 40;
    bad += same(a, "accept_draws.reserved", "reserved");
    for (uint32_t t : {2u, 0xffffffffu}) {
        a = good.without;
        a.timepoints = t;
        bad += same(a, "accept_draws.timepoints", "timepoints above 1");
    }
    for (uint32_t n : {0u, 65u, 0xffffffffu}) {
        a = good.without;
        a.n_targets = n;
        bad += same(a, "accept_draws.n_targets", "n_targets");
    }
    a = good.without;
    a.target_hists = nullptr;
    bad += same(a, "target_hists is NULL", "NULL target_hists");
    std::vector<uint64_t> holed = good.hists;
    for (uint32_t b = 0; b < kBins; ++b) holed[(size_t)63 * kBins + b] = 0;
    a = good.without;
    a.target_hists = holed.data();
    bad += same(a, "target_hists[63] is empty", "an all-zero row");
    a = good.without;
    a.sample_cells = nullptr;
    bad += same(a, "sample_cells is NULL", "NULL sample_cells");
    for (uint32_t m : {0u, kKeep + 1u, 0xffffffffu}) {
        std::vector<uint32_t> cc = good.cells;
        cc[17] = m;
        a = good.without;
        a.sample_cells = cc.data();
        bad += same(a, "sample_cells[17]", "a size out of range");
    }
    for (uint32_t d : {0u, 65u}) {
        a = good.without;
        a.n_draws = d;
        bad += same(a, "accept_draws.n_draws", "n_draws");
    }
    a = good.without;
    a.first_draw = 63;
    a.n_draws = 2;
    bad += same(a, "first_draw + n_draws", "a range past draw 63");
    a = good.without;
    a.n_targets = 3;
    a.timepoint_mask = 0b1000;
    bad += same(a, "timepoint_mask has bits at or above T = 3", "mask bits at T");
    bad += same(good.without, "n_replicates must be < 2^32", "2^32 replicates", 0, 1ull << 32);
    // the keys' 32-bit bound: n x n_draws, not n
    bad += expect(inv(good.without, 0, (1ull << 26) - 1u), nullptr, "2^26 - 1 replicates on 64 draws");
    bad += expect(inv(good.without, 0, 1ull << 26), "select_draws: n_replicates x n_draws = 4294967296 must be < 2^32",
                  "2^26 replicates on 64 draws");
    a = good.without;
    a.n_draws = 63;
    bad += expect(inv(a, 0, 1ull << 26), nullptr, "2^26 replicates on 63 draws");
    a.n_draws = 1;
    bad += expect(inv(a, 0, (1ull << 32) - 1u), nullptr, "2^32 - 1 replicates on one draw");
    bad += expect(ad::invalid(kBins, kKeep, 0, 1ull << 26, good.with), nullptr, "accept_draws has no such bound");

    // the rank rules of ecdna_ssa_select_t
    const uint64_t ranks[33] = {1, 2, 3, ~0ull, 5};
    uint64_t ones[33];
    double fr[33];
    for (int j = 0; j < 33; ++j) ones[j] = 1u, fr[j] = 1.0 / (j + 1);
    bad += expect(sd::invalid_ranks(5, ranks, nullptr), nullptr, "five ranks");
    bad += expect(sd::invalid_ranks(6, ranks, nullptr), "select_draws.ranks[5] must be >= 1", "a rank of 0");
    bad += expect(sd::invalid_ranks(32, ones, nullptr), nullptr, "32 ranks");
    bad += expect(sd::invalid_ranks(32, nullptr, fr), nullptr, "32 fractions");
    for (uint32_t K : {0u, 33u, 0xffffffffu})
        bad += expect(sd::invalid_ranks(K, ones, nullptr), "select_draws.n_ranks must be in [1, 32]", "K");
    bad += expect(sd::invalid_ranks(3, ones, fr), "exactly one of select_draws.ranks and select_draws.fractions", "both");
    bad += expect(sd::invalid_ranks(3, nullptr, nullptr), "exactly one of select_draws.ranks and select_draws.fractions",
                  "neither");
    for (double f : {0.0, -0.5, std::nextafter(1.0, 2.0), std::nan(""), std::numeric_limits<double>::infinity()}) {
        fr[2] = f;
        bad += expect(sd::invalid_ranks(3, nullptr, fr), "select_draws.fractions[2] must be in (0, 1]", "a fraction");
    }
    fr[2] = 1.0;
    bad += expect(sd::invalid_ranks(3, nullptr, fr), nullptr, "a fraction of 1");

    // the rules of a digit pass
    bad += expect(sd::invalid_pass(0, 1, ones, ones), nullptr, "pass 0");
    bad += expect(sd::invalid_pass(7, 32, ones, ones), nullptr, "pass 7, 32 prefixes");
    bad += expect(sd::invalid_pass(8, 1, ones, ones), "select_draws_digits.pass must be in [0, 7]", "pass 8");
    for (uint32_t K : {0u, 33u})
        bad += expect(sd::invalid_pass(0, K, ones, ones), "select_draws_digits.n_prefixes must be in [1, 32]", "K");
    bad += expect(sd::invalid_pass(0, 1, nullptr, ones), "select_draws_digits.prefixes is NULL", "NULL prefixes");
    bad += expect(sd::invalid_pass(0, 1, ones, nullptr), "select_draws_digits.out_hist is NULL", "NULL out_hist");
    if (bad) return 1;
    std::puts("validate ok");
    return 0;
}

static int print_bytes() {
    const Good good;
    const struct {
        uint64_t n;
        uint32_t draws;
    } shapes[] = {{1ull << 20, 64}, {131072, 64}, {258, 3}, {1ull << 26, 64}, {(1ull << 26) - 1u, 64}};
    for (const auto& s : shapes) {
        ecdna_ssa_accept_draws_t a = good.without;
        a.n_draws = s.draws;
        std::printf("n %llu draws %u n_keys %llu keys %llu hist %llu cdf %llu scalars %llu taken %d\n",
                    (unsigned long long)s.n, s.draws, (unsigned long long)sd::n_keys(s.n, s.draws),
                    (unsigned long long)sd::keys_bytes(s.n, s.draws), (unsigned long long)sd::hist_bytes(),
                    (unsigned long long)sd::cdf_bytes(4, 1025), (unsigned long long)sd::scalars_bytes(4),
                    (int)sd::invalid(kBins, kKeep, 0, s.n, a).empty());
    }
    return 0;
}

static int check_same() {
    Good good;
    ecdna_ssa_accept_draws_t a = good.without;
    a.n_targets = 3;
    a.timepoint_mask = 0b101;
    a.first_draw = 61;
    a.n_draws = 3;
    const sd::Block b = sd::remember(a, kBins);
    int bad = 0;
    auto differs = [&](const ecdna_ssa_accept_draws_t& x, const char* what) {
        if (sd::same(b, x, kBins)) bad += std::fprintf(stderr, "reported as the same block: %s\n", what), 1;
    };
    if (!sd::same(b, a, kBins)) bad += std::fprintf(stderr, "the block itself differs\n"), 1;
    // copies of what the block points to at other addresses: the same block
    std::vector<uint64_t> hists(good.hists.begin(), good.hists.begin() + 3 * kBins);
    std::vector<uint32_t> cells(good.cells.begin(), good.cells.begin() + 3);
    ecdna_ssa_accept_draws_t c = a;
    c.target_hists = hists.data();
    c.sample_cells = cells.data();
    if (!sd::same(b, c, kBins)) bad += std::fprintf(stderr, "equal copies differ\n"), 1;
    // ... and the remembered block holds copies of its own: the caller's arrays may change afterwards
    cells[2] += 1u;
    differs(c, "a changed size");
    cells[2] -= 1u;
    hists[2 * kBins + 4] += 1u;
    differs(c, "a changed target bin");
    hists[2 * kBins + 4] -= 1u;
    if (!sd::same(b, c, kBins)) bad += std::fprintf(stderr, "the restored copies differ\n"), 1;
    ecdna_ssa_accept_draws_t x = c;
    x.timepoint_mask = 0b111;
    differs(x, "a changed mask");
    x = c;
    x.timepoint_mask = 0;
    differs(x, "mask 0");
    x = c;
    x.first_draw = 60;
    differs(x, "a changed first draw");
    x = c;
    x.n_draws = 2;
    differs(x, "a changed number of draws");
    x = c;
    x.n_targets = 2;
    differs(x, "fewer targets");
    x = c;
    x.timepoints = 1;
    differs(x, "the other store");
    good.cells[1] = 7;  // (the arrays the block was remembered from)
    differs(a, "the caller's own array changed after the keys were made");
    if (sd::same(b, c, kBins + 1u)) bad += std::fprintf(stderr, "another number of bins is the same\n"), 1;
    if (sd::same(sd::Block{}, c, kBins)) bad += std::fprintf(stderr, "an empty block is the same\n"), 1;
    if (bad) return 1;
    std::puts("same ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "validate") == 0) return check_validate();
    if (argc > 1 && std::strcmp(argv[1], "bytes") == 0) return print_bytes();
    if (argc > 1 && std::strcmp(argv[1], "same") == 0) return check_same();
    std::fprintf(stderr, "usage: select_draws_check validate | bytes | same\n");
    return 2;
}
