// ssa_thinwave.hpp — a wave's work on one kept sample, shared by the thinning passes over the kept samples: ssa_thin.hip,
// ssa_accept_draws.hip, ssa_pool_draws.hip and ssa_select_draws.hip (thinning mapping v1 and the three mappings over
// its draws, include/ecdna_ssa.h). ssa_rescore.hip keeps its own copy of the scan: through wave_kept_hist it measured
// half a percent slower (docs/PERF_LOG.md). The wave's LDS, the kept sample as its header gives it, the one scan
// into the full histogram, one thinned draw, the record of a group on the whole or the thinned sample, and the
// acceptance rule on such a record. The passes perform the same operations in the same order through these, which is
// what makes a thinned record, a verdict or a pool one pass's as much as another's: the histograms and the sums are
// integers, and the f64 operations on them are wave_cohort_record's (ssa_wave.hpp), fp contract off.
// Plain functions over one 64-lane wave; every lane of the wave calls the wave_ functions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

// The wave's share of the dynamic LDS, wave_words u32 words (thin_waves' plan: 2 * bins + scratch_words;
// pool_draws_wave_words'): the kept sample's full histogram, a thinned sample's, and the scratch that holds the table of
// drawn positions while a sample is drawn and the scored sample's CDF while it is scored, as in ssa_cohort: one is dead
// while the other lives. Every term of wave_words is even, so each wave's scratch is 8-byte aligned for the CDF.
struct ThinLds {
    uint32_t* fh;   // [bins] the kept sample's histogram
    uint32_t* wh;   // [bins] a thinned sample's
    uint32_t* tab;  // [scratch_words]: the table, or
    double* F;      // [bins] the scored sample's CDF
};
__device__ __forceinline__ ThinLds thin_lds(unsigned long long* lds, uint32_t wave, uint32_t wave_words, uint32_t bins) {
    uint32_t* fh = reinterpret_cast<uint32_t*>(lds) + (size_t)wave * wave_words;
    uint32_t* tab = fh + 2u * bins;
    return {fh, fh + bins, tab, reinterpret_cast<double*>(tab)};
}

// The kept sample at index `at` of a store of m cells per sample: header {a, b}, a N- cells and the b true copy numbers
// of row. guard: the guard ended the replicate and left no sample. As a population it is "a N- cells, then the row" (no
// bin counters): the shape of a snapshot's population, rows only.
struct KeptSample {
    bool guard;
    uint32_t nm, np;  // N- cells; the cells of the row (a row holds m cells)
    uint64_t cells_all;
    const uint16_t* row;
    SamplePop pop;
};
__device__ __forceinline__ KeptSample kept_sample(const uint2* headers, const uint16_t* cells, uint64_t at, uint32_t m) {
    const uint2 h = headers[at];
    const uint32_t np = min(h.y, m);
    const uint16_t* row = cells + at * m;
    return {h.x == kKeptGuard && h.y == kKeptGuard, h.x, np, (uint64_t)h.x + np, row,
            SamplePop{(uint64_t)h.x, nullptr, 0u, 0u, row, np}};
}

// The one scan: the kept sample's full histogram into fh[bins] (N- cells in bin 0, true copy numbers clipped at the last
// bin), the row read with u16 loads (a row of m cells is not 16-byte aligned when m is odd). Returns the wave's sum of k.
__device__ __forceinline__ uint64_t wave_kept_hist(uint32_t* fh, uint32_t bins, const KeptSample& k, uint32_t lane) {
    const uint32_t last = bins - 1u;
    for (uint32_t b = lane; b < bins; b += 64u) fh[b] = 0u;
    wave_sync_lds();
    uint64_t ksum = 0;
    for (uint32_t j = lane; j < k.np; j += 64u) {
        const uint32_t kk = k.row[j];
        atomicAdd(&fh[kk < last ? kk : last], 1u);
        ksum += kk;
    }
    if (lane == 0) atomicAdd(&fh[0], k.nm);
    wave_sync_lds();
    return wave_sum(ksum);
}

// One thinned sample of the kept sample into L.wh: subsample mapping v1's over the population (wave_sample_picks<0>) under
// `key`, the key the kept sample was drawn under, on stream `tag` (thin::stream_tag). The picks are counted into zeros,
// or taken out of a copy of the full histogram L.fh (a complement). psum: the wave's sum of k over the picked positions.
// Returns true when the guard ends the draw: wh is then not to be used. plan is neither whole nor bad.
__device__ __forceinline__ bool wave_thin_draw(const ThinLds& L, uint32_t table_slots, uint32_t bins, const KeptSample& k,
                                               const SamplePlan& plan, uint32_t tag, uint64_t key, uint64_t rid,
                                               uint32_t lane, uint64_t& psum) {
    for (uint32_t b = lane; b < bins; b += 64u) L.wh[b] = plan.comp ? L.fh[b] : 0u;
    wave_sync_lds();
    psum = 0;
    const bool bad = wave_sample_picks<0>(L.wh, L.tab, table_slots, k.pop, plan.N, plan.mp, plan.comp, bins - 1u, tag, rid,
                                          (uint32_t)key, (uint32_t)(key >> 32), lane, psum);
    wave_sync_lds();
    psum = wave_sum(psum);
    return bad;
}

// The records of a group's targets list[0 .. count) on the whole kept sample (L.fh) or on the thinned sample of m1 cells
// wave_thin_draw left in L.wh: lane j < count returns the j-th target's (wave_cohort_record). ksum: wave_kept_hist's.
__device__ __forceinline__ ecdna_rep_stats_t wave_thin_record(const ThinLds& L, uint32_t bins, const KeptSample& k,
                                                              bool whole, bool comp, uint32_t m1, uint64_t ksum,
                                                              uint64_t psum, const double* target_cdf,
                                                              const double* target_scalars, const uint32_t* list,
                                                              uint32_t count, uint32_t lane) {
    const uint32_t* hh = whole ? L.fh : L.wh;
    const uint64_t cells = whole ? k.cells_all : (uint64_t)m1;
    const uint64_t ks_sum = whole ? ksum : (comp ? ksum - psum : psum);
    const uint64_t nplus_s = whole ? (uint64_t)k.np : cells - (uint64_t)L.wh[0];
    return wave_cohort_record(hh, L.F, bins, cells, ks_sum, nplus_s, target_cdf, target_scalars, list, count, lane);
}

// ssa_accept_mask's rule: a tie passes; +inf switches the statistic off, NaN distances included; a NaN distance fails
// every finite threshold. A record the guards zero has four zero distances and passes every row.
__device__ __forceinline__ bool passes(double d, double thr) { return thr == __builtin_huge_val() || d <= thr; }
__device__ __forceinline__ bool row_passes(const ecdna_rep_stats_t& rec, const double* thr) {
    return passes(rec.ks, thr[0]) && passes(rec.mean_rel, thr[1]) && passes(rec.entropy_rel, thr[2]) &&
           passes(rec.frequency_diff, thr[3]);
}

// Rule 1 for replicate q: the error word of its one summary, or of every participating phase's (AcceptArgs).
__device__ __forceinline__ uint32_t draws_error(const DrawsArgs& s, uint32_t q) {
    if (s.err_stride == 0u) return s.summaries[q].error;
    uint32_t err = 0u;
    for (uint32_t t = 0; t < s.n_slices; ++t)
        if ((s.slice_mask >> t) & 1ull) err |= s.summaries[(uint64_t)q + t * s.err_stride].error;
    return err;
}

// The call's draws first_draw .. first_draw + n_draws - 1 as a 64-bit set.
__device__ __forceinline__ uint64_t draws_range(const DrawsArgs& s) {
    return (s.n_draws >= 64u ? ~0ull : (1ull << s.n_draws) - 1ull) << s.first_draw;
}

}  // namespace ecdna
