// ssa_passage.hip — the phase boundary of a serial-passage run (ecdna_ssa_passages_t; gfx950).
//
// The reference's cell-line strategy restarts growth from the subsample: a culture is grown, a few hundred cells are
// taken and measured, and those same cells found the next flask. At the end of growth phase g this pass draws each
// replicate's sample of m cells by subsample mapping v1 under the phase's key seed_g (include/ecdna_ssa.h, DESIGN.md
// §3.4), writes the sample's ecdna_rep_stats_t and the per-set sum of the samples' histograms exactly as
// ssa_subsample.hip does (the phase's "measurement"), and, unless the phase is the last, materialises the sample as
// the founders of phase g + 1: {n-, n+} per replicate and the n+ true copy numbers in ascending order, which is the
// order an initial histogram gives the steppers' replicate start.
//
// One wave per replicate. Per wave in LDS: the replicate's histogram wh (u32 per bin), the inclusive prefix sums of its
// bin counters pre (position -> copy number), the table of drawn positions tab, and the founders fs (u16, a power of
// two >= 64 slots padded with 0xffff for the sort). The draws, the table and the lookup are ssa_sampledraw.hpp's.
//  - sample = the picks (m' = m): every new pick of an N+ position appends its copy number (wave_sample_picks).
//  - complement (m' = N - m, so N <= 2m): the positions are walked once, those not in the table are the sample.
//  - m >= N: every position.
// The founders are then ordered by a bitonic sort of the wave over the first pow2ceil(n+) slots. A sample the guard
// ended (all-zero statistics) founds the empty population, as does an empty one.
// The samples' non-zero bins go to global memory directly: a workgroup histogram beside 2,048 bins and m = 4096 would
// not fit 64 KiB of LDS.
//
// The keep pass (ecdna_ssa_keep_t, keep mapping v1) is the same kernel's KEEP instance: the sample of the end-of-run
// population is materialised in the founder format — the same picks, complement walk, whole population, sort and
// {n-, n+} header — into the run's kept buffers, and nothing else: no statistics, no pooled histogram (the sample's
// records are made later, from the kept cells, by ssa_rescore). A sample the guard ended keeps the header
// {0xffffffff, 0xffffffff} instead of the empty population.
//
// The timepoint keep block (ecdna_ssa_keep_timepoints_t, timepoint keep mapping v1) keeps the sample of every timepoint
// of a longitudinal run with the same body. A passage context launches the KEEP instance above once per phase, under
// the phase's key, into slice g of the run's buffers. A snapshot context launches the KEEP = 2 instance after
// ssa_snapstats, while the chunk's snapshot rows exist: one wave per (replicate, snapshot) pair, the population a row
// only, the draws on snapshot s's stream, slice s of the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssa_device.hpp"
#include "ssa_launch.h"
#include "ssa_sampledraw.hpp"
#include "ssa_wave.hpp"

#pragma clang fp contract(off)

namespace ecdna {

namespace {

constexpr uint32_t kPasBlock = 256;
constexpr uint32_t kPasPad = 0xffffu;

// fs[0 .. P) ascending, P a power of two >= 64: the wave's bitonic network, 64 compare-exchanges per step.
__device__ __forceinline__ void wave_bitonic_sort_u16(uint16_t* fs, uint32_t P, uint32_t lane) {
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint16_t x = fs[i], y = fs[l];
                    const bool up = (i & k) == 0u;
                    if ((x > y) == up) {
                        fs[i] = y;
                        fs[l] = x;
                    }
                }
            }
            wave_sync_lds();
        }
    }
}

// BAG as in ssa_hist: 0 = rows only; 1 / 2 = u16 / u32 bin counters bags[q][bag_k] for copy numbers 1..bag_k plus
// the large-k cells at the head of the row.
// KEEP: 1 = the keep pass (founder_rows / founder_counts are the kept cells and headers; stats, sample_hist and target
// are not read). 2 = the snapshot keep pass (ecdna_ssa_keep_timepoints_t, timepoint keep mapping v1; BAG = 0): the same
// body over the chunk's (replicate, snapshot) pairs, one wave per pair. Pair w = q * n_snap + s is the population
// "nminus N- cells, then snapshot row w" of ssa_snapstats, sampled on the stream of snapshot s as ssa_snapstats samples
// it, and kept in slice s of the run's buffers. A snapshot that was not taken is the empty population.
template <int BAG, int KEEP>
__global__ void __launch_bounds__(kPasBlock) ssa_passage(const PassageArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const ChunkIds& ids = a.ids;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nw = blockDim.x >> 6;
    const uint32_t wave_words = ids.bins + a.state.bag_k + a.table_slots + (a.sort_slots >> 1);
    uint32_t* wh = lds + (size_t)wave * wave_words;                   // [bins]
    uint32_t* pre = wh + ids.bins;                                    // [bag_k]
    uint32_t* tab = pre + a.state.bag_k;                              // [table_slots]
    uint16_t* fs = reinterpret_cast<uint16_t*>(tab + a.table_slots);  // [sort_slots]
    const uint32_t r_begin = blockIdx.x * ids.reps_per_block;
    if (r_begin >= ids.n) return;
    const uint32_t r_end = min(ids.n, r_begin + ids.reps_per_block);
    const uint32_t last = ids.bins - 1;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const bool want = a.founder_rows != nullptr;
    const uint32_t fcap = min(a.m, a.sort_slots);  // a founder row is never written past m

    // populations per replicate: its snapshots in the snapshot keep pass, else its final state. (w below n * n_snap
    // fits u32: the chunk holds a row of at least 128 bytes per pair; launch_keep_snapshots checks it.)
    const uint32_t S = KEEP == 2 ? a.n_snap : 1u;
    for (uint32_t w = r_begin * S + wave; w < r_end * S; w += nw) {
        const uint32_t q = KEEP == 2 ? w / S : w;       // the replicate
        const uint32_t t = KEEP == 2 ? w - q * S : 0u;  // its snapshot
        uint64_t nm;
        uint32_t np;
        if (KEEP == 2) {  // as ssa_snapstats reads a pair: the row is never read past its memory
            const ecdna_snapshot_t* meta = a.snap_meta + w;
            const bool taken = meta->taken != 0u;
            nm = taken ? meta->nminus : 0ull;
            np = taken ? (uint32_t)min(meta->nplus, a.state.row_stride) : 0u;
        } else {
            const ecdna_rep_summary_t* s = a.state.summaries + q;
            nm = s->nminus;
            np = (uint32_t)s->nplus;
        }
        const uint64_t rid = ids.rid0 + (uint64_t)q * ids.rid_stride;
        const uint64_t set = rid / ids.reps_per_set;
        SamplePlan plan = sample_plan(a.m, nm + (uint64_t)np);
        if (want)  // (ordered before the founders are appended by the fence of step 1)
            for (uint32_t b = lane; b < a.sort_slots; b += 64u) fs[b] = (uint16_t)kPasPad;

        // 1. counters: prefix sums for the position -> k lookup, and (whole / complement) the full histogram
        uint64_t ksum = 0;  // sum of k over the full population (need_full)
        // (row w of a.state: the replicate's row, or the pair's snapshot row — a row-only population, bag_k = 0)
        const SamplePop pop = wave_load_final_state<BAG>(a.state, w, nm, np, ids.bins, plan, wh, pre, ksum, lane);

        // 2.-4. draws until m' distinct positions have appeared; every new one is looked up and counted (and, when the
        // picks are the sample, gathered as a founder)
        uint64_t psum = 0;  // sum of k over the picked positions
        uint32_t gn = 0;    // founders gathered (N+ cells)
        bool bad = plan.bad;
        if (!plan.whole && !bad)
            bad = wave_sample_picks<BAG>(wh, tab, a.table_slots, pop, plan.N, plan.mp, plan.comp, last,
                                         sample_stream_tag(KEEP == 2 ? t + 1u : 0u), rid, k0, k1, lane, psum,
                                         want ? fs : nullptr, fcap, &gn);
        wave_sync_lds();

        // founders of a whole population or of a complement: one walk over the positions (N <= 2m), from the 64-block
        // that holds the first N+ position on
        bool fbad = bad;
        if (want && !bad && plan.need_full) {
            const SampleTable tb = sample_table(plan.mp);
            bool lane_bad = false;
            for (uint32_t base = (uint32_t)min(nm, (uint64_t)plan.N) & ~63u; base < plan.N; base += 64u) {
                const uint32_t v = base + lane;
                bool keep = v < plan.N && (plan.whole || !sample_tab_has(tab, tb, v));
                uint32_t kk = 0;
                if (keep && !sample_pos_k<BAG>(pop, v, kk)) {
                    lane_bad = true;
                    keep = false;
                }
                wave_append_u16(keep && kk > 0u, kk, fs, fcap, gn, lane);
            }
            fbad = __any(lane_bad);
            wave_sync_lds();
        }

        // 5. statistics of the sample histogram, its bins added to the set's sample histogram in global memory
        const uint32_t nminus_s = wh[0];  // the sample's N- cells (whole: all of them; complement: those left)
        if (!KEEP)
            wave_sample_stats(plan, bad, a.m, nm + (uint64_t)np, np, ksum, psum, wh,
                              reinterpret_cast<unsigned long long*>(a.sample_hist + set * ids.bins), ids.bins, a.target,
                              lane, a.stats + q);

        // 6. the founders, ascending
        if (want) {
            if (fbad || gn > fcap) gn = 0;  // (gn > fcap: more N+ cells than a sample holds, unreachable)
            if (gn > 1u) {
                uint32_t P = 64u;
                while (P < gn) P <<= 1;
                wave_bitonic_sort_u16(fs, P, lane);
            }
            // (the snapshot keep pass: slice t of the run's buffers)
            const uint64_t at = KEEP == 2 ? (uint64_t)t * a.slice_stride + q : (uint64_t)q;
            uint16_t* out = a.founder_rows + at * a.founder_stride;
            for (uint32_t j = lane; j < gn; j += 64u) out[j] = fs[j];
            if (lane == 0)
                a.founder_counts[at] =
                    KEEP && fbad ? make_uint2(kKeptGuard, kKeptGuard) : make_uint2(fbad ? 0u : nminus_s, gn);
        }
        wave_sync_lds();  // wh and fs are reset for the wave's next replicate
    }
}

}  // namespace

hipError_t launch_passage(const PassageArgs& a, uint32_t blocks, hipStream_t stream) {
    PassageArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = passage_waves(a.ids.bins, a.state.bag_k, a.table_slots, a.sort_slots, &lds);
    if (lds > kPassLdsMax || a.m > a.founder_stride || a.sort_slots < 64u || (a.sort_slots & (a.sort_slots - 1u)))
        return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_passage<0, 0>, (const void*)ssa_passage<1, 0>,
                                         (const void*)ssa_passage<2, 0>};
    return hipLaunchKernel(table[bag_index(a.state)], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

hipError_t launch_keep(const PassageArgs& a, uint32_t blocks, hipStream_t stream) {
    PassageArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = keep_waves(a.ids.bins, a.state.bag_k, a.table_slots, a.sort_slots, &lds);
    // (a kept row is m cells: the kernel never writes a row past min(m, sort_slots))
    if (lds > kPassLdsMax || !a.founder_rows || !a.founder_counts || a.m > a.founder_stride || a.sort_slots < 64u ||
        (a.sort_slots & (a.sort_slots - 1u)))
        return hipErrorInvalidValue;
    static const void* const table[3] = {(const void*)ssa_passage<0, 1>, (const void*)ssa_passage<1, 1>,
                                         (const void*)ssa_passage<2, 1>};
    return hipLaunchKernel(table[bag_index(a.state)], dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

hipError_t launch_keep_snapshots(const PassageArgs& a, uint32_t blocks, hipStream_t stream) {
    PassageArgs copy = a;
    void* args[] = {&copy};
    size_t lds = 0;
    const uint32_t nw = keep_snapshots_waves(a.ids.bins, a.table_slots, a.sort_slots, &lds);
    // (a row-only population: no counters and no summaries; the pair index and its step stay below 2^32; a slice holds
    // the chunk's replicates)
    if (lds > kPassLdsMax || !a.founder_rows || !a.founder_counts || a.m > a.founder_stride || a.sort_slots < 64u ||
        (a.sort_slots & (a.sort_slots - 1u)) || a.state.bags || a.state.bag_k || !a.state.rows || !a.snap_meta ||
        a.n_snap < 1u || a.n_snap > kMaxSnapshots || (uint64_t)a.ids.n * a.n_snap + 4u > 0xffffffffull ||
        a.slice_stride < a.ids.n)
        return hipErrorInvalidValue;
    return hipLaunchKernel((const void*)ssa_passage<0, 2>, dim3(blocks), dim3(nw * 64u), args, lds, stream);
}

}  // namespace ecdna
