// TEST INFRASTRUCTURE ONLY — host-side check of the bin stepper's branch-free segregation popcount over the event's
// own words (ecdna-evo_amd/csrc/ssa_device.hpp, popcount_base_words) against a restatement of the first loop of
// WordStream::binomial_half_with (w3 and the spares, word by word), built with hipcc for the host and run on the CPU
// by tests/test_three_word_popcount.py.
//
// For nsp = 0, 1, 2 spares in hand the words in hand hold all of n exactly where n <= 32 + 32 * nsp (the stepper
// calls the function for 65 <= n <= 96 with two spares); there the loop below consumes the whole of n from w3 and
// the first ceil(n / 32) - 1 spares, and both must agree, with the stream position the stepper sets, (n + 63) >> 5.
// Also checked: the value does not depend on the words it must not read (the spares past those n covers, and the
// bits above n's last one).
// Prints "cases=<n> mismatches=<m>"; exits 1 on any mismatch.
#include <stdint.h>
#include <stdio.h>

#include "ssa_device.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint32_t popc(uint32_t x) {
    uint32_t c = 0;
    for (; x; x &= x - 1u) ++c;
    return c;
}

// binomial_half_with's first loop from pos = 1 (w2 went to the pick): returns the count; `left` is what the Philox
// blocks would still have to supply and `pos` the stream position afterwards
uint32_t first_loop(uint32_t n, uint32_t w3, uint32_t s0, uint32_t s1, uint32_t nsp, uint32_t& left, uint32_t& pos) {
    uint32_t c = 0;
    pos = 1;
    while (n && pos < 2u + nsp) {
        const uint32_t p = pos++;
        const uint32_t w = p < 2u ? w3 : (p == 2u ? s0 : s1);
        const uint32_t take = n < 32u ? n : 32u;
        const uint32_t mask = take == 32u ? 0xffffffffu : ((1u << take) - 1u);
        c += popc(w & mask);
        n -= take;
    }
    left = n;
    return c;
}

}  // namespace

int main() {
    long cases = 0, bad = 0;
    const uint32_t fixed[2] = {0u, 0xffffffffu};
    for (uint32_t nsp = 0; nsp <= 2u; ++nsp) {
        for (uint32_t n = 1; n <= 96u; ++n) {
            for (int rep = 0; rep < 8 + 2000; ++rep) {
                uint32_t w3, s0, s1;
                if (rep < 8) {  // every all-ones / all-zero combination of the three words
                    w3 = fixed[rep & 1];
                    s0 = fixed[(rep >> 1) & 1];
                    s1 = fixed[(rep >> 2) & 1];
                } else {
                    const uint64_t a = next_u64(), b = next_u64();
                    w3 = (uint32_t)a;
                    s0 = (uint32_t)(a >> 32);
                    s1 = (uint32_t)b;
                }
                uint32_t left, pos;
                const uint32_t want = first_loop(n, w3, s0, s1, nsp, left, pos);
                const bool fast = n <= 32u + 32u * nsp;  // the words in hand cover n
                if (fast != (left == 0u)) {
                    ++bad;
                    fprintf(stderr, "limit: n %u nsp %u fast %d left %u\n", n, nsp, (int)fast, left);
                    continue;
                }
                if (!fast) continue;  // the general path draws it
                ++cases;
                const uint32_t got = ecdna::popcount_base_words(w3, s0, s1, n);
                // the words and bits it must not read, flipped
                const uint32_t words = (n + 31u) >> 5;
                const uint32_t topbits = (n & 31u) ? ~((1u << (n & 31u)) - 1u) : 0u;
                const uint32_t w3x = w3 ^ (words == 1u ? topbits : 0u);
                const uint32_t s0x = words < 2u ? ~s0 : s0 ^ (words == 2u ? topbits : 0u);
                const uint32_t s1x = words < 3u ? ~s1 : s1 ^ topbits;
                const uint32_t got_x = ecdna::popcount_base_words(w3x, s0x, s1x, n);
                if (got != want || got_x != want || pos != ((n + 63u) >> 5)) {
                    if (++bad <= 5)
                        fprintf(stderr, "mismatch: n %u nsp %u words %08x %08x %08x: loop %u (pos %u) header %u / %u\n", n,
                                nsp, w3, s0, s1, want, pos, got, got_x);
                }
            }
        }
    }
    printf("cases=%ld mismatches=%ld\n", cases, bad);
    return bad ? 1 : 0;
}
