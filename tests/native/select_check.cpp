// select_check.cpp — the host side of ecdna_ssa_ctx_select (ecdna-evo_amd/csrc/ssa_select.hpp) on the CPU, for
// tests/test_select_native.py: the key map the kernels call and the select driver ssa_api_passes.cpp calls. Built for
// the host alone, with the address and undefined-behaviour sanitizers.
//
//   select_check edges    checks on a list of edge doubles (0, the smallest denormal, 1 - ulp, 1, the largest finite,
//                         +inf, NaN, and their negatives) that the key is monotone, that key(value(key)) is the key and
//                         that -0.0 and every NaN are mapped as select mapping v1 says; prints "edges ok"
//   select_check          reads one case from stdin and prints its order statistics. Input, one line each:
//                           ranks k1 k2 ...          or          fractions f1 f2 ...
//                           bits b b b ...     four lines, one per distance: the population's values as the hex bit
//                                              patterns of their doubles (all four lines equally long)
//                         It makes the keys with key_of and runs the engine's driver (select::run) with a pass that
//                         builds the histograms [4][K][256] of the walk's prefixes as the engine does (dedup, key_top,
//                         key_digit); what it prints is what the driver wrote to its four outputs.
//                         Output: "population M", "ranks ...", and per distance "values <hex bits> ..." and
//                         "counts ...".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "ssa_select.hpp"

namespace sel = ecdna::select;

static uint64_t bits_of(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

static int check_edges() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double up[] = {0.0, 5e-324, 1.0 - 0x1p-53, 1.0, std::numeric_limits<double>::max(), inf, nan};
    std::vector<double> edge;
    for (int i = 5; i > 0; --i) edge.push_back(-up[i]);  // -inf .. -denormal
    for (double d : up) edge.push_back(d);
    for (size_t i = 0; i + 1 < edge.size(); ++i)
        if (!(sel::key_of(edge[i]) < sel::key_of(edge[i + 1])))
            return std::fprintf(stderr, "key not monotone at edge %zu\n", i), 1;
    for (double d : edge) {
        const uint64_t k = sel::key_of(d);
        if (sel::key_of_bits(sel::bits_of_key(k)) != k) return std::fprintf(stderr, "key(value(key)) != key\n"), 1;
        if (d == d && sel::bits_of_key(k) != bits_of(d)) return std::fprintf(stderr, "value(key(d)) != d\n"), 1;
        if (k == sel::kExcluded) return std::fprintf(stderr, "a number has the excluded key\n"), 1;
    }
    if (sel::key_of(-0.0) != sel::key_of(0.0) || sel::bits_of_key(sel::key_of(-0.0)) != 0)
        return std::fprintf(stderr, "-0.0 is not +0.0\n"), 1;
    if (sel::key_of(0.0) != sel::kSignBit) return std::fprintf(stderr, "key(0.0)\n"), 1;
    const uint64_t nans[] = {0x7FF0000000000001ull, 0xFFF8000000000000ull, 0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};
    for (uint64_t b : nans)
        if (sel::key_of_bits(b) != 0xFFF8000000000000ull || sel::bits_of_key(sel::key_of_bits(b)) != sel::kQuietNaN)
            return std::fprintf(stderr, "a NaN is not the canonical one\n"), 1;
    if (!(sel::key_of(inf) < sel::key_of(nan) && sel::key_of(nan) < sel::kExcluded)) return 1;
    if (sel::key_top(0x123456789ABCDEF0ull, 0) != 0 || sel::key_top(0x123456789ABCDEF0ull, 3) != 0x123456ull ||
        sel::key_digit(0x123456789ABCDEF0ull, 0) != 0x12 || sel::key_digit(0x123456789ABCDEF0ull, 7) != 0xF0)
        return std::fprintf(stderr, "key_top / key_digit\n"), 1;
    std::puts("edges ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "edges") == 0) return check_edges();
    std::vector<uint64_t> ranks;
    std::vector<double> fractions;
    std::vector<std::vector<uint64_t>> keys;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string kind, w;
        if (!(words >> kind)) continue;
        if (kind == "ranks") {
            while (words >> w) ranks.push_back(std::strtoull(w.c_str(), nullptr, 10));
        } else if (kind == "fractions") {
            while (words >> w) fractions.push_back(std::strtod(w.c_str(), nullptr));
        } else if (kind == "bits") {
            keys.emplace_back();
            while (words >> w) {
                const uint64_t b = std::strtoull(w.c_str(), nullptr, 16);
                double d;
                std::memcpy(&d, &b, sizeof d);
                keys.back().push_back(sel::key_of(d));
            }
        } else {
            return std::fprintf(stderr, "select_check: unknown line '%s'\n", kind.c_str()), 2;
        }
    }
    const uint32_t K = (uint32_t)(ranks.empty() ? fractions.size() : ranks.size());
    if (keys.size() != sel::kDistances || K < 1 || K > sel::kMaxRanks || (!ranks.empty() && !fractions.empty()))
        return std::fprintf(stderr, "select_check: four bits lines and 1 .. 32 ranks or fractions\n"), 2;
    for (const auto& k : keys)
        if (k.size() != keys[0].size()) return std::fprintf(stderr, "select_check: bits lines differ in length\n"), 2;

    // one pass's histograms [4][K][256] of the walk's prefixes [4][kMaxRanks], from the host's keys
    auto host_pass = [&](uint32_t pass, const uint64_t* prefixes, uint64_t* hist) {
        for (uint32_t x = 0; x < sel::kDistances; ++x) {
            uint64_t top[sel::kMaxRanks], unique[sel::kMaxRanks];
            uint32_t group[sel::kMaxRanks];
            for (uint32_t j = 0; j < K; ++j) top[j] = sel::key_top(prefixes[x * sel::kMaxRanks + j], pass);
            const uint32_t G = sel::dedup(top, K, unique, group);
            std::vector<uint64_t> table((size_t)G * sel::kDigits, 0ull);  // the device's table of distinct prefixes
            for (const uint64_t key : keys[x])
                for (uint32_t g = 0; g < G; ++g)
                    if (sel::key_top(key, pass) == unique[g]) ++table[g * sel::kDigits + sel::key_digit(key, pass)];
            for (uint32_t j = 0; j < K; ++j)
                for (uint32_t d = 0; d < sel::kDigits; ++d)
                    hist[((size_t)x * K + j) * sel::kDigits + d] = table[group[j] * sel::kDigits + d];
        }
        return 0;
    };
    uint64_t population = 0;
    std::vector<uint64_t> out_ranks(K), counts((size_t)sel::kDistances * K);
    std::vector<double> values((size_t)sel::kDistances * K);
    if (sel::run(K, ranks.empty() ? nullptr : ranks.data(), fractions.empty() ? nullptr : fractions.data(), host_pass,
                 &population, out_ranks.data(), values.data(), counts.data()))
        return std::fprintf(stderr, "select_check: the driver returned an error\n"), 1;
    std::printf("population %" PRIu64 "\nranks", population);
    for (uint32_t j = 0; j < K; ++j) std::printf(" %" PRIu64, out_ranks[j]);
    std::printf("\n");
    for (uint32_t x = 0; x < sel::kDistances; ++x) {
        std::printf("values");
        for (uint32_t j = 0; j < K; ++j) std::printf(" %016" PRIx64, bits_of(values[(size_t)x * K + j]));
        std::printf("\ncounts");
        for (uint32_t j = 0; j < K; ++j) std::printf(" %" PRIu64, counts[(size_t)x * K + j]);
        std::printf("\n");
    }
    return 0;
}
