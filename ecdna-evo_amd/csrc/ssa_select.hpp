// ssa_select.hpp — the host side of ecdna_ssa_ctx_select / ecdna_ssa_ctx_select_digits (select mapping v1,
// include/ecdna_ssa.h): the order-preserving key of a distance and its inverse, the rank walk of the 8-bit radix
// select over the per-pass digit histograms, the driver that runs the passes and writes the outputs (select::run, which
// ecdna_ssa_ctx_select and ecdna_ssa_ctx_select_draws call in ssa_api_passes.cpp), and the rank and digit-pass rules of
// both calls. No HIP runtime call and nothing of the API: the key functions are the ones the kernels of ssa_select.hip
// call, and the walk and the driver are pure, so all are checked on a machine without a GPU
// (tests/native/select_check.cpp, tests/test_select_native.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace ecdna {
namespace select {

constexpr uint32_t kPasses = 8;        // 8 bits of the 64-bit key per pass, most significant first
constexpr uint32_t kDigits = 256;
constexpr uint32_t kMaxRanks = 32;     // K: ranks of a call, and so prefixes (groups) of a pass
constexpr uint32_t kDistances = 4;     // ks, mean_rel, entropy_rel, frequency_diff
constexpr uint64_t kSignBit = 0x8000000000000000ull;
constexpr uint64_t kQuietNaN = 0x7FF8000000000000ull;
constexpr uint64_t kPlusInf = 0x7FF0000000000000ull;
// The key of a replicate outside the population. No number has it: the largest key is key(NaN) = 0xFFF8000000000000,
// as every NaN is mapped to the canonical one first.
constexpr uint64_t kExcluded = ~0ull;

// key(d) from d's bits: -0.0 -> +0.0, any NaN -> the canonical quiet NaN, then the sign bit flipped for a clear sign
// and every bit for a set one. a < b as numbers iff key(a) < key(b); NaN sorts above +inf.
__host__ __device__ inline uint64_t key_of_bits(uint64_t b) {
    if ((b & ~kSignBit) > kPlusInf) b = kQuietNaN;
    if (b == kSignBit) b = 0;
    return (b & kSignBit) ? ~b : (b ^ kSignBit);
}
__host__ __device__ inline uint64_t key_of(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, sizeof b);
    return key_of_bits(b);
}
// The bits of the number a key stands for (key_of_bits(bits_of_key(k)) == k for every key of a number).
__host__ __device__ inline uint64_t bits_of_key(uint64_t k) { return (k & kSignBit) ? (k ^ kSignBit) : ~k; }
inline double value_of_key(uint64_t k) {
    const uint64_t b = bits_of_key(k);
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

// The top 8 * pass bits of a key, shifted down (0 in pass 0), and the 8 bits after them.
__host__ __device__ inline uint64_t key_top(uint64_t key, uint32_t pass) { return pass ? key >> (64u - 8u * pass) : 0ull; }
__host__ __device__ inline uint32_t key_digit(uint64_t key, uint32_t pass) {
    return (uint32_t)(key >> (56u - 8u * pass)) & 255u;
}

// k = max(1, ceil(f * M)) in f64, for f in (0, 1].
inline uint64_t rank_of_fraction(double f, uint64_t M) {
    const double x = __builtin_ceil(f * (double)M);
    const uint64_t k = x >= 18446744073709551616.0 ? ~0ull : (uint64_t)x;
    return k < 1u ? 1u : k;
}

// One step of the walk. hist[256] counts, by their digit of this pass, the keys that share the top 8 * pass bits of
// `prefix`; `remaining` (1 .. their number) is the wanted key's rank among them and `less` the number of keys below
// them all. The digit is the smallest whose cumulative count reaches `remaining`; the step returns the prefix with
// that digit set, the rank among the keys that share it, the keys below those, and their number (after the last
// pass: the keys equal to the wanted one, so counts_le = less + count).
struct Step {
    uint64_t prefix, remaining, less, count;
};
inline Step walk_step(const uint64_t* hist, uint32_t pass, uint64_t prefix, uint64_t remaining, uint64_t less) {
    uint64_t cum = 0;
    uint32_t d = 0;
    while (d + 1u < kDigits && cum + hist[d] < remaining) cum += hist[d++];
    const uint32_t shift = 56u - 8u * pass;
    const uint64_t kept = pass ? prefix & (~0ull << (shift + 8u)) : 0ull;
    return {kept | ((uint64_t)d << shift), remaining - cum, less + cum, hist[d]};
}

// The walk of K ranks over the four distances. start(), then per pass: prefixes() are the pass's input
// (ecdna_ssa_ctx_select_digits' [4][K]) and feed() takes its histograms [4][K][256], summed over the shards. Pass 0's
// row sum is the population M, which turns fractions into ranks. A rank above M (every rank when M = 0) is "over": its
// value is +inf and its counts_le M.
struct Walk {
    uint32_t K = 0, pass = 0;
    bool by_fraction = false;
    uint64_t M = 0;
    double fraction[kMaxRanks] = {};
    uint64_t rank[kMaxRanks] = {};
    uint64_t prefix[kDistances][kMaxRanks] = {}, remaining[kDistances][kMaxRanks] = {}, less[kDistances][kMaxRanks] = {},
             count[kDistances][kMaxRanks] = {};

    void start(uint32_t n_ranks, const uint64_t* ranks, const double* fractions) {
        *this = Walk();
        K = n_ranks;
        by_fraction = ranks == nullptr;
        for (uint32_t j = 0; j < K; ++j) {
            if (by_fraction) fraction[j] = fractions[j];
            else rank[j] = ranks[j];
        }
    }
    bool over(uint32_t j) const { return rank[j] > M; }
    bool done() const { return pass == kPasses; }
    const uint64_t* prefixes() const { return &prefix[0][0]; }  // [4][kMaxRanks]: row x, entries 0 .. K - 1
    // hist[x][j][d], j < K (rows of K, not kMaxRanks)
    void feed(const uint64_t* hist) {
        if (pass == 0) {
            M = 0;
            for (uint32_t d = 0; d < kDigits; ++d) M += hist[d];
            for (uint32_t j = 0; j < K; ++j) {
                if (by_fraction) rank[j] = rank_of_fraction(fraction[j], M);
                for (uint32_t x = 0; x < kDistances; ++x) remaining[x][j] = rank[j];
            }
        }
        for (uint32_t x = 0; x < kDistances; ++x)
            for (uint32_t j = 0; j < K; ++j) {
                if (over(j)) continue;
                const Step s = walk_step(hist + ((uint64_t)x * K + j) * kDigits, pass, prefix[x][j], remaining[x][j],
                                         less[x][j]);
                prefix[x][j] = s.prefix;
                remaining[x][j] = s.remaining;
                less[x][j] = s.less;
                count[x][j] = s.count;
            }
        ++pass;
    }
    // after the last pass
    uint64_t key(uint32_t x, uint32_t j) const { return over(j) ? key_of_bits(kPlusInf) : prefix[x][j]; }
    double value(uint32_t x, uint32_t j) const { return value_of_key(key(x, j)); }
    uint64_t counts_le(uint32_t x, uint32_t j) const { return over(j) ? M : less[x][j] + count[x][j]; }
};

// The distinct values among top[0 .. K): unique[0 .. return) in order of first appearance, group[j] = top[j]'s place in
// it. The kernel matches a key against each distinct prefix once.
inline uint32_t dedup(const uint64_t* top, uint32_t K, uint64_t* unique, uint32_t* group) {
    uint32_t G = 0;
    for (uint32_t j = 0; j < K; ++j) {
        uint32_t g = 0;
        while (g < G && unique[g] != top[j]) ++g;
        if (g == G) unique[G++] = top[j];
        group[j] = g;
    }
    return G;
}

#pragma GCC visibility push(hidden)  // (host-side helpers of the library's own units: not for its symbol table)

// The rank rules of ecdna_ssa_select_t, as the message of ECDNA_E_INVALID ("" for ranks the engine takes). who: the
// prefix the call's arguments are named under, "select" or "select_draws".
inline std::string invalid_ranks(const std::string& who, uint32_t n_ranks, const uint64_t* ranks,
                                 const double* fractions) {
    if (n_ranks < 1u || n_ranks > kMaxRanks) return who + ".n_ranks must be in [1, 32]";
    if ((ranks != nullptr) == (fractions != nullptr))
        return "exactly one of " + who + ".ranks and " + who + ".fractions must be given";
    for (uint32_t j = 0; j < n_ranks; ++j) {
        if (ranks && ranks[j] == 0u) return who + ".ranks[" + std::to_string(j) + "] must be >= 1";
        if (fractions && !(fractions[j] > 0.0 && fractions[j] <= 1.0))
            return who + ".fractions[" + std::to_string(j) + "] must be in (0, 1] and not NaN";
    }
    return "";
}

// The rules of one digit pass, likewise. who: "select_digits" or "select_draws_digits".
inline std::string invalid_pass(const std::string& who, uint32_t pass, uint32_t n_prefixes, const void* prefixes,
                                const void* out_hist) {
    if (pass >= kPasses) return who + ".pass must be in [0, 7]";
    if (n_prefixes < 1u || n_prefixes > kMaxRanks) return who + ".n_prefixes must be in [1, 32]";
    if (!prefixes) return who + ".prefixes is NULL";
    if (!out_hist) return who + ".out_hist is NULL";
    return "";
}

// The whole select of K ranks (or fractions): the eight digit passes, each fed to the walk, then the four outputs
// (any may be NULL): the population, the ranks [K], and the values and counts_le [4][K]. pass(pass_index, prefixes,
// hist_out) -> int fills hist_out [4][K][256] for the prefixes [4][kMaxRanks] (a pass that writes nothing leaves
// zeros: an empty population); the first non-zero code it returns ends the select and is returned.
template <class Pass>
int run(uint32_t K, const uint64_t* ranks, const double* fractions, Pass pass, uint64_t* out_population,
        uint64_t* out_ranks, double* out_values, uint64_t* out_counts_le) {
    Walk walk;
    walk.start(K, ranks, fractions);
    std::vector<uint64_t> hist((uint64_t)kDistances * K * kDigits, 0ull);
    while (!walk.done()) {
        if (const int rc = pass(walk.pass, walk.prefixes(), hist.data())) return rc;
        walk.feed(hist.data());
    }
    if (out_population) *out_population = walk.M;
    for (uint32_t j = 0; j < K; ++j) {
        if (out_ranks) out_ranks[j] = walk.rank[j];
        for (uint32_t x = 0; x < kDistances; ++x) {
            if (out_values) out_values[(uint64_t)x * K + j] = walk.value(x, j);
            if (out_counts_le) out_counts_le[(uint64_t)x * K + j] = walk.counts_le(x, j);
        }
    }
    return 0;
}

#pragma GCC visibility pop

}  // namespace select
}  // namespace ecdna
