// ssa_sampledraw.hpp — subsample mapping v1 (include/ecdna_ssa.h) for one population, shared by the
// end-of-run sample (ssa_subsample.hip), the phase boundary of a passage run (ssa_passage.hip) and the samples at the
// snapshots (ssa_snapstats.hip). The draws: the Lemire draw below N on a tagged Philox stream, the wave's table of the
// positions drawn so far, and the position -> copy number lookup (wave_sample_picks). Around them: which positions
// are drawn for a sample of m cells (sample_plan), the population's histogram and prefix sums from the final state
// (wave_row_hist, wave_load_final_state) and the sample's statistics (wave_sample_stats).
// One 64-lane wave per population; every lane of the wave calls the wave_ functions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

constexpr uint32_t kSubEmpty = 0xffffffffu;
constexpr uint32_t kSubTag = 0xC0000000u;      // Philox counter word 1 of draw block t: kSubTag | stream | t
constexpr uint32_t kSubMaxDraws = 1u << 16;    // the guard: draws per population
constexpr uint32_t kSubMaxBlocks = 1024;       // Philox blocks per draw (each rejects with p < 2^-4: unreachable)

// The stream field of counter word 1: 0 for the end-of-run sample, (s + 1) << 16 for the sample at snapshot s
// (t < kSubMaxBlocks = 2^10 and s < kMaxSnapshots = 64, so the fields never meet and stay below kSubTag's bits).
__host__ __device__ constexpr uint32_t sample_stream_tag(uint32_t snapshot_plus_one) {
    return kSubTag | (snapshot_plus_one << 16);
}

// Draw i of replicate (rid_lo, rid_hi): a Lemire draw below N. Philox block t = 0, 1, ... on counter
// (i, tag | t, rid lo, rid hi); its four words are tried in order, word x gives p = x * N and is accepted as
// p >> 32 when the low half is >= thr = (2^32 - N) mod N.
__device__ __forceinline__ uint32_t sub_draw(uint32_t i, uint32_t N, uint32_t thr, uint32_t tag, uint32_t rid_lo,
                                             uint32_t rid_hi, uint32_t k0, uint32_t k1, bool& fail) {
    for (uint32_t t = 0; t < kSubMaxBlocks; ++t) {
        const uint4 w = philox4x32_10(make_uint4(i, tag | t, rid_lo, rid_hi), k0, k1);
        const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t p = (uint64_t)x[j] * N;
            if ((uint32_t)p >= thr) return (uint32_t)(p >> 32);
        }
    }
    fail = true;
    return 0u;
}

// A population of N = nm + (N+ cells) cells in download order: positions 0 .. nm - 1 are the N- cells, then `small`
// cells held in bin counters (BAG: pre[bag_k] their inclusive prefix sums, in the wave's LDS), then row[0 .. nrow).
struct SamplePop {
    uint64_t nm;
    const uint32_t* pre;
    uint32_t bag_k;
    uint32_t small;
    const uint16_t* row;
    uint32_t nrow;
};

// Position v (below N) -> copy number kk, in download order: the N- cells (kk = 0), the counters k ascending, the row.
// False for a position the counters and the row cannot account for.
template <int BAG>
__device__ __forceinline__ bool sample_pos_k(const SamplePop& pop, uint32_t v, uint32_t& kk) {
    kk = 0;
    if ((uint64_t)v < pop.nm) return true;
    const uint32_t u = v - (uint32_t)pop.nm;
    if (BAG && u < pop.small) {
        uint32_t lo = 0, hi = pop.bag_k - 1u;  // the first b with pre[b] > u
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pop.pre[mid] > u)
                hi = mid;
            else
                lo = mid + 1u;
        }
        kk = lo + 1u;
        return true;
    }
    const uint32_t j = u - pop.small;
    if (j >= pop.nrow) return false;
    kk = pop.row[j];
    return true;
}

// What is drawn for a sample of m cells of a population of cells_all: the sample is the whole population (m >= N, no
// draws), the mp = m picked positions, or what mp = N - m < m picked positions leave (comp). need_full: the sample is
// made from the population's full histogram. bad: positions are u32 and 0xffffffff marks an empty table slot.
struct SamplePlan {
    bool whole, bad;
    uint32_t N, mp;
    bool comp, need_full;
};
__device__ __forceinline__ SamplePlan sample_plan(uint32_t m, uint64_t cells_all) {
    const bool whole = (uint64_t)m >= cells_all;
    const bool bad = !whole && cells_all >= 0xffffffffull;
    const uint32_t N = (uint32_t)cells_all;
    const uint32_t mp = (whole || bad) ? 0u : min(m, N - m);
    const bool comp = mp != m;
    return {whole, bad, N, mp, comp, whole || comp};
}

// row[0 .. n) counted into the wave's histogram wh (bins clip at `last`), 16 bytes (8 cells) per lane and load; ksum
// gains the lane's sum of k. LDS atomics only: the caller orders them against its plain accesses of wh.
__device__ __forceinline__ void wave_row_hist(const uint16_t* row, uint32_t n, uint32_t last, uint32_t* wh,
                                              uint64_t& ksum, uint32_t lane) {
    for (uint32_t c = lane * 8u; c < n; c += 512u) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + c);
        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (c + (uint32_t)j < n) {
                const uint32_t kk = (wv[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                atomicAdd(&wh[kk < last ? kk : last], 1u);
                ksum += kk;
            }
        }
    }
}

// Step 1 of the mapping for replicate q of a final state (nm, np: its summary's N- and N+ cells): wh[bins] is zeroed;
// the bin counters give pre[bag_k] and, when plan.need_full, enter wh and ksum; the cells the row holds follow
// (never trust counters past the row, nor the summary past the row's memory: counters that hold more cells than the
// summary set plan.bad), and lane 0 adds the N- cells. Returns the population for the lookup.
// The one fence inside orders the plain stores that zero wh (and whatever plain LDS stores the caller made just before
// the call, ssa_passage's founder padding) before other lanes' atomics on wh; pre is written plainly and wh by atomics
// after it, so the caller fences (wave_sample_picks does, after clearing its table) before wh or pre are read.
template <int BAG>
__device__ __forceinline__ SamplePop wave_load_final_state(const FinalState& fs, uint32_t q, uint64_t nm, uint32_t np,
                                                           uint32_t bins, SamplePlan& plan, uint32_t* wh, uint32_t* pre,
                                                           uint64_t& ksum, uint32_t lane) {
    const uint32_t last = bins - 1u;
    const uint16_t* row = fs.rows + (uint64_t)q * fs.row_stride;
    for (uint32_t b = lane; b < bins; b += 64u) wh[b] = 0u;
    wave_sync_lds();
    uint32_t small = 0;
    if (BAG) {
        for (uint32_t base = 0; base < fs.bag_k; base += 64u) {
            const uint32_t b = base + lane;
            const uint32_t cnt = b < fs.bag_k ? bag_counter<BAG>(fs.bags, q, fs.bag_k, b) : 0u;
            if (plan.need_full && cnt) {
                const uint32_t kk = b + 1u;
                atomicAdd(&wh[kk < last ? kk : last], cnt);
                ksum += (uint64_t)kk * cnt;
            }
            const uint32_t scan = wave_inclusive_scan(cnt, lane);
            if (b < fs.bag_k) pre[b] = small + scan;
            small += __shfl(scan, 63, 64);
        }
        if (!plan.whole && small > np) plan.bad = true;
    }
    const uint32_t nrow = (uint32_t)min((uint64_t)(np >= small ? np - small : 0u), fs.row_stride);
    if (plan.need_full) {
        wave_row_hist(row, nrow, last, wh, ksum, lane);
        if (lane == 0) atomicAdd(&wh[0], (uint32_t)nm);
    }
    return {nm, pre, fs.bag_k, small, row, nrow};
}

// The wave's table of drawn positions for m' picks: 2 * pow2ceil(m') slots (load <= 1/2), hashed by the top bits of a
// multiplicative hash, linear probing.
struct SampleTable {
    uint32_t tsize;
    uint32_t sh;
};
__device__ __forceinline__ SampleTable sample_table(uint32_t mp) {
    const uint32_t lg = mp > 1u ? 32u - (uint32_t)__clz(mp - 1u) : 0u;
    return {2u << lg, 31u - lg};
}
// Whether position v was picked (the table as wave_sample_picks left it).
__device__ __forceinline__ bool sample_tab_has(const uint32_t* tab, SampleTable t, uint32_t v) {
    uint32_t sl = (v * 0x9E3779B1u) >> t.sh;
    for (uint32_t probe = 0; probe < t.tsize; ++probe) {
        const uint32_t old = tab[sl];
        if (old == v) return true;
        if (old == kSubEmpty) return false;
        sl = (sl + 1u) & (t.tsize - 1u);
    }
    return false;
}

// Appends the copy numbers of the lanes with `take` to out[0 .. cap) behind the n already there (wave-uniform n; the
// order within a batch is lane order). Every lane of the wave calls it.
__device__ __forceinline__ void wave_append_u16(bool take, uint32_t kk, uint16_t* out, uint32_t cap, uint32_t& n,
                                                uint32_t lane) {
    const unsigned long long mask = __ballot(take);
    if (take) {
        const uint32_t idx = n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (idx < cap) out[idx] = (uint16_t)kk;
    }
    n += (uint32_t)__popcll(mask);
}

// Steps 2-4 of the mapping: draws on stream `tag` until mp distinct positions below N have appeared; every new one is
// looked up and counted into the wave's histogram wh (bins clip at `last`; comp: taken out of it, the picked cells
// are those left out of the sample). psum gains the lane's sum of k over its picked positions. tab[table_slots] is
// the wave's table of drawn positions (LDS). Returns true when the guard ends the population (too small a table, 2^16
// draws, a position the counters and the row cannot account for): wh is then not to be used.
// gout (ssa_passage.hip; nullptr: off): the true copy numbers of the picked N+ cells are appended to gout[0 .. gcap),
// *gn counting them (the picks are the sample, comp == false; a complement's cells are gathered by its caller).
template <int BAG>
__device__ __forceinline__ bool wave_sample_picks(uint32_t* wh, uint32_t* tab, uint32_t table_slots,
                                                  const SamplePop& pop, uint32_t N, uint32_t mp, bool comp,
                                                  uint32_t last, uint32_t tag, uint64_t rid, uint32_t k0, uint32_t k1,
                                                  uint32_t lane, uint64_t& psum, uint16_t* gout = nullptr,
                                                  uint32_t gcap = 0, uint32_t* gn = nullptr) {
    const SampleTable tb = sample_table(mp);
    const uint32_t tsize = tb.tsize, sh = tb.sh;
    bool bad = tsize > table_slots;
    const uint32_t tclear = bad ? 0u : tsize;
    for (uint32_t b = lane; b < tclear; b += 64u) tab[b] = kSubEmpty;
    wave_sync_lds();
    const uint32_t thr = (0u - N) % N;
    const uint32_t rid_lo = (uint32_t)rid, rid_hi = (uint32_t)(rid >> 32);
    bool lane_bad = false;
    uint32_t count = bad ? mp : 0u, base = 0;
    while (count < mp && base < kSubMaxDraws) {
        // the next draws, one per lane: at most as many as positions are still missing, so every new
        // draw of the batch is one of the first m' and the table never holds more than m' positions
        const uint32_t nact = min(64u, min(mp - count, kSubMaxDraws - base));
        const bool active = lane < nact;
        uint32_t v = kSubEmpty;
        if (active) v = sub_draw(base + lane, N, thr, tag, rid_lo, rid_hi, k0, k1, lane_bad);
        // a draw that repeats an earlier one of its batch is not new, whichever lane reaches LDS first
        bool dup = false;
        for (uint32_t j = 0; j + 1u < nact; ++j) {
            const uint32_t vj = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
            dup = dup || (j < lane && vj == v);
        }
        // the others are distinct: each is new iff the table did not hold it before the batch
        bool isnew = false;
        if (active && !dup && !lane_bad) {
            uint32_t sl = (v * 0x9E3779B1u) >> sh;
            bool placed = false;
            for (uint32_t probe = 0; probe < tsize; ++probe) {
                const uint32_t old = atomicCAS(&tab[sl], kSubEmpty, v);
                if (old == kSubEmpty || old == v) {
                    isnew = old == kSubEmpty;
                    placed = true;
                    break;
                }
                sl = (sl + 1u) & (tsize - 1u);
            }
            if (!placed) lane_bad = true;
        }
        uint32_t kk = 0;
        bool counted = false;
        if (isnew) {
            counted = sample_pos_k<BAG>(pop, v, kk);
            if (counted) {
                const uint32_t bin = kk < last ? kk : last;
                if (comp)
                    atomicSub(&wh[bin], 1u);
                else
                    atomicAdd(&wh[bin], 1u);
                psum += kk;
            } else {
                lane_bad = true;
            }
        }
        if (gout && !comp) wave_append_u16(counted && kk > 0u, kk, gout, gcap, *gn, lane);
        count += (uint32_t)__popcll(__ballot(isnew));
        base += nact;
        wave_sync_lds();
    }
    return bad || count < mp || __any(lane_bad);
}

// Step 5 of the mapping: the statistics of the sample whose histogram wh holds (the full histogram, the picks, or the
// full histogram less the picks), written to *out; its non-zero bins are added to `sums` (a workgroup histogram in LDS
// or the set's row in global memory). ksum / psum: the lanes' sums of k over the full population / the picked positions.
// bad (the guard, or a state the counters cannot account for): all-zero statistics, nothing added to sums.
// Reads wh plainly and fences nothing: the caller's wave_sync_lds after the last atomics on wh comes before the call,
// and another before wh is written again.
__device__ __forceinline__ void wave_sample_stats(const SamplePlan& plan, bool bad, uint32_t m, uint64_t cells_all,
                                                  uint32_t np, uint64_t ksum, uint64_t psum, const uint32_t* wh,
                                                  unsigned long long* sums, uint32_t bins, const StatsTarget& target,
                                                  uint32_t lane, ecdna_rep_stats_t* out) {
    ksum = wave_sum(ksum);
    psum = wave_sum(psum);
    if (bad) {
        if (lane == 0) *out = ecdna_rep_stats_t{};
    } else {
        const uint64_t cells = plan.whole ? cells_all : (uint64_t)m;
        const uint64_t ks_sum = plan.whole ? ksum : (plan.comp ? ksum - psum : psum);
        const uint64_t nplus_s = plan.whole ? (uint64_t)np : cells - (uint64_t)wh[0];
        wave_rep_stats(wh, sums, bins, cells, ks_sum, nplus_s, target.has, target.cdf, target.mean, target.entropy,
                       target.freq, lane, out);
    }
}

}  // namespace ecdna
