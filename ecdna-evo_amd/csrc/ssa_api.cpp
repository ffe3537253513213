// ssa_api.cpp — the C ABI of include/ecdna_ssa.h: parameter validation,
// device-resident run contexts, chunking by HBM capacity, and launches of the
// stepper and end-of-run kernels (ssa_kernels.hip, ssa_hist.hip, ssa_subsample.hip, ssa_snapstats.hip,
// ssa_passage.hip, ssa_cohort.hip), of the post-launch acceptance pass (ssa_accept.hip) and of the passes over the kept
// samples (ssa_rescore.hip, ssa_thin.hip, ssa_accept_draws.hip, ssa_pool_draws.hip, ssa_select_draws.hip). The kept samples of the keep block and of the timepoint keep block lie in one kind of store
// (KeptStore), and every pass over them has one implementation, which the two blocks' entry points call.
//
// This file replaces, for one GPU, the per-replicate driver loop of the
// reference: run_simulations(idx) mapped by rayon over seed*10 .. seed*10+runs
// (src/main.rs:55-225). Everything here is host code; there is no CPU
// fallback — without a gfx950 device every entry point returns
// ECDNA_E_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ecdna_ssa.h"
#include "ssa_accept_draws.hpp"
#include "ssa_pool_draws.hpp"
#include "ssa_select_draws.hpp"
#include "ssa_cohort.hpp"
#include "ssa_keep.hpp"
#include "ssa_launch.h"
#include "ssa_plan.hpp"
#include "ssa_select.hpp"
#include "ssa_thin.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// TRY(expr): return from the calling function with the error of a failed step, which is either a HIP call (the
// error is recorded here, with the call's text) or a function of this file that returns an ECDNA_* code (and has
// recorded its own).
int rc_of(int rc, const char*) { return rc; }
int rc_of(hipError_t e, const char* what) {
    if (e == hipSuccess) return ECDNA_OK;
    return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define TRY(expr)                                         \
    do {                                                  \
        if (int _rc = rc_of((expr), #expr)) return _rc;   \
    } while (0)

struct InitOfSet {
    const uint16_t* copies;
    uint64_t nplus;
    uint64_t nminus;
};

InitOfSet init_of_set(const ecdna_ssa_params_t* p, uint64_t s) {
    InitOfSet r;
    if (p->init_set_offsets) {
        r.copies = p->init_copies + p->init_set_offsets[s];
        r.nplus = p->init_set_offsets[s + 1] - p->init_set_offsets[s];
    } else {
        r.copies = p->init_copies;
        r.nplus = p->init_nplus;
    }
    r.nminus = p->init_set_nminus ? p->init_set_nminus[s] : p->init_nminus;
    return r;
}

// The index of the first of `count` target histograms ([count][bins]) without a cell; count if there is none, or no
// targets at all.
uint32_t first_empty_target(const uint64_t* hists, uint32_t count, uint32_t bins) {
    for (uint32_t i = 0; hists && i < count; ++i) {
        const uint64_t* t = hists + (uint64_t)i * bins;
        if (std::all_of(t, t + bins, [](uint64_t x) { return x == 0; })) return i;
    }
    return count;
}

// The step between the global ids of a call's replicates (replicate_stride = 0 stands for 1).
uint64_t rid_stride(const ecdna_ssa_params_t& p) { return p.replicate_stride ? p.replicate_stride : 1u; }

int validate(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext, const ecdna_ssa_passages_t* pas) {
    if (!p) return fail(ECDNA_E_INVALID, "params is NULL");
    if (!p->rates || p->n_param_sets == 0) return fail(ECDNA_E_INVALID, "rates/n_param_sets");
    for (uint32_t s = 0; s < p->n_param_sets; ++s) {  // (the steppers' f32 time-step division relies on it)
        const ecdna_rates_t& r = p->rates[s];
        for (const float x : {r.b0, r.b1, r.d0, r.d1})
            if (!(x == 0.f || (x >= 0x1p-60f && x <= 0x1p60f)))
                return fail(ECDNA_E_INVALID, "rates must be 0 or in [2^-60, 2^60]");
    }
    if (p->reps_per_set == 0) return fail(ECDNA_E_INVALID, "reps_per_set must be >= 1");
    if (p->reserved0) return fail(ECDNA_E_INVALID, "reserved0 must be 0");
    if (p->reserved1) return fail(ECDNA_E_INVALID, "reserved1 must be 0");
    if (p->subsample_cells && !(p->flags & ECDNA_FLAG_REP_STATS))
        return fail(ECDNA_E_INVALID, "subsample_cells needs ECDNA_FLAG_REP_STATS");
    if (p->subsample_cells > ecdna::kMaxSubsampleCells)
        return fail(ECDNA_E_INVALID, "subsample_cells must be <= 4096");
    // (bit 31 is the library's internal snapshot bit, kFlagSnapshotsRt: a caller setting it, or any other unknown bit,
    // would silently select another kernel instance)
    if (p->flags & ~(uint32_t)ECDNA_FLAG_ALL) return fail(ECDNA_E_INVALID, "unknown bits in flags");
    if (p->hist_bins < 2 || p->hist_bins > ecdna::kMaxHistBins)
        return fail(ECDNA_E_INVALID, "hist_bins must be in [2, 4096]");
    if ((p->flags & ECDNA_FLAG_REP_STATS) && p->hist_bins > 2048)
        return fail(ECDNA_E_INVALID, "ECDNA_FLAG_REP_STATS needs hist_bins <= 2048");
    if (p->process != ECDNA_PURE_BIRTH && p->process != ECDNA_BIRTH_DEATH)
        return fail(ECDNA_E_INVALID, "unknown process");
    if (p->segregation < 0 || p->segregation > 3) return fail(ECDNA_E_INVALID, "unknown segregation");
    if (p->max_iter > 0xffffffffull) return fail(ECDNA_E_INVALID, "max_iter must be < 2^32");
    if (p->n_replicates > 0xffffffffull) return fail(ECDNA_E_INVALID, "n_replicates must be < 2^32 per call");
    const uint64_t stride = rid_stride(*p);
    if (p->n_replicates && (p->n_replicates - 1) > (~0ull - p->first_replicate) / stride)
        return fail(ECDNA_E_INVALID, "replicate ids overflow u64");
    if (p->n_replicates && (p->first_replicate + (p->n_replicates - 1) * stride) / p->reps_per_set >= p->n_param_sets)
        return fail(ECDNA_E_INVALID, "replicate ids map past the last parameter set");
    if (p->cell_cap == 0) return fail(ECDNA_E_INVALID, "cell_cap must be >= 1");
    if ((p->flags & ECDNA_FLAG_REFERENCE_DRAWS) && (p->flags & ECDNA_FLAG_BIN_STORE))
        return fail(ECDNA_E_INVALID, "ECDNA_FLAG_REFERENCE_DRAWS runs the row store only (no ECDNA_FLAG_BIN_STORE)");
    if ((p->flags & ECDNA_FLAG_BIN_STORE) && p->bin_kmax != 0 && p->bin_kmax != 32 && p->bin_kmax != 64 &&
        p->bin_kmax != 256)
        return fail(ECDNA_E_INVALID, "bin_kmax must be 0 (= 64), 32, 64 or 256");
    if (p->n_snapshots > ecdna::kMaxSnapshots) return fail(ECDNA_E_INVALID, "at most 64 snapshots");
    if (p->n_snapshots && !p->snapshot_cells) return fail(ECDNA_E_INVALID, "snapshot_cells is NULL");
    for (uint32_t q = 1; q < p->n_snapshots; ++q)
        if (p->snapshot_cells[q] < p->snapshot_cells[q - 1])
            return fail(ECDNA_E_INVALID, "snapshot_cells must be sorted ascending");
    if (!p->init_copies && (p->init_nplus || p->init_set_offsets))
        return fail(ECDNA_E_INVALID, "init_copies is NULL");
    for (uint32_t s = 0; s < p->n_param_sets; ++s) {
        InitOfSet in = init_of_set(p, s);
        if (in.nplus > p->cell_cap) return fail(ECDNA_E_INVALID, "initial N+ cells exceed cell_cap");
        if ((p->flags & ECDNA_FLAG_BIN_STORE) && p->big_cap) {
            const uint32_t kmax = p->bin_kmax ? p->bin_kmax : 64u;
            uint64_t big = 0;
            for (uint64_t j = 0; j < in.nplus; ++j) big += in.copies[j] > kmax;
            if (big > p->big_cap) return fail(ECDNA_E_INVALID, "initial cells above bin_kmax exceed big_cap");
        }
        // (populations are u32: the bin stepper adds n- + n+ in 32 bits, and a sum of 2^32 would wrap past max_cells)
        if (in.nminus > 0xffffffffull || in.nminus + in.nplus > 0xffffffffull)
            return fail(ECDNA_E_INVALID, "initial cells (N- plus N+) must be < 2^32");
        for (uint64_t j = 0; j < in.nplus; ++j)
            if (in.copies[j] == 0) return fail(ECDNA_E_INVALID, "initial copy numbers must be >= 1");
        if (!p->init_set_offsets && !p->init_set_nminus) break;
    }
    if (ext) {  // the extension block (per-snapshot ABC statistics)
        if (ext->struct_size != sizeof(ecdna_ssa_ext_t))
            return fail(ECDNA_E_INVALID, "ext.struct_size must be sizeof(ecdna_ssa_ext_t)");
        if (ext->reserved) return fail(ECDNA_E_INVALID, "ext.reserved must be 0");
        if (ext->snapshot_subsample_cells > ecdna::kMaxSubsampleCells)
            return fail(ECDNA_E_INVALID, "ext.snapshot_subsample_cells must be <= 4096");
        if (ext->snapshot_stats > 1u) return fail(ECDNA_E_INVALID, "ext.snapshot_stats must be 0 or 1");
        if (ext->snapshot_stats) {
            if (!p->n_snapshots) return fail(ECDNA_E_INVALID, "ext.snapshot_stats needs n_snapshots > 0");
            if (!(p->flags & ECDNA_FLAG_REP_STATS))
                return fail(ECDNA_E_INVALID, "ext.snapshot_stats needs ECDNA_FLAG_REP_STATS");
            const uint32_t q = first_empty_target(ext->snapshot_target_hists, p->n_snapshots, p->hist_bins);
            if (q < p->n_snapshots)
                return fail(ECDNA_E_INVALID, "ext.snapshot_target_hists[" + std::to_string(q) + "] is empty");
        }
    }
    if (pas) {  // the passage block (serial passaging)
        if (pas->struct_size != sizeof(ecdna_ssa_passages_t))
            return fail(ECDNA_E_INVALID, "passages.struct_size must be sizeof(ecdna_ssa_passages_t)");
        if (pas->reserved) return fail(ECDNA_E_INVALID, "passages.reserved must be 0");
        if (pas->n_passages < 1u || pas->n_passages > ecdna::kMaxPassages)
            return fail(ECDNA_E_INVALID, "passages.n_passages must be in [1, 16]");
        if (pas->passage_cells < 1u || pas->passage_cells > ecdna::kMaxSubsampleCells)
            return fail(ECDNA_E_INVALID, "passages.passage_cells must be in [1, 4096]");
        if (pas->passage_cells > p->cell_cap)
            return fail(ECDNA_E_INVALID, "passages.passage_cells must be <= cell_cap");
        if (!(p->flags & ECDNA_FLAG_REP_STATS)) return fail(ECDNA_E_INVALID, "passages need ECDNA_FLAG_REP_STATS");
        if (p->subsample_cells)
            return fail(ECDNA_E_INVALID, "passages: subsample_cells must be 0 (passage_cells is the sample size)");
        if (p->n_snapshots) return fail(ECDNA_E_INVALID, "passages: n_snapshots must be 0");
        if (ext && ext->snapshot_stats) return fail(ECDNA_E_INVALID, "passages: ext.snapshot_stats must be 0");
        if (p->flags & ECDNA_FLAG_REFERENCE_DRAWS)
            return fail(ECDNA_E_INVALID, "passages do not run under ECDNA_FLAG_REFERENCE_DRAWS");
        const uint32_t g = first_empty_target(pas->passage_target_hists, pas->n_passages, p->hist_bins);
        if (g < pas->n_passages)
            return fail(ECDNA_E_INVALID, "passages.passage_target_hists[" + std::to_string(g) + "] is empty");
    }
    return ECDNA_OK;
}

// The Philox key of growth phase g of a passage run (passage mapping v1, include/ecdna_ssa.h): the seed itself for
// phase 0, else the splitmix64 finaliser of seed + g * 0x9E3779B97F4A7C15.
uint64_t passage_seed(uint64_t seed, uint32_t g) {
    if (g == 0) return seed;
    uint64_t z = seed + (uint64_t)g * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Reference draws (ECDNA_FLAG_REFERENCE_DRAWS): rand_core 0.6.4 seed_from_u64 — the 32-byte ChaCha key filled
// by a PCG32 sequence from the seed (little-endian words).
void chacha_key_from_u64(uint64_t state, uint32_t key[8]) {
    const uint64_t mul = 6364136223846793005ull, inc = 11634580027462260723ull;
    for (int i = 0; i < 8; ++i) {
        state = state * mul + inc;
        const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
        const uint32_t rot = (uint32_t)(state >> 59);
        key[i] = (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
    }
}

// rand_distr 0.4.3 BTPE setup of Binomial(n, 1/2) (the step-0 constants; oracle/ssa_compat.c computes the same
// per call), one row of refdraws::kBtpeRow doubles per copy number k = n / 2: npq, m, p1, x_m, x_l, x_r, c,
// p2, lambda_l, lambda_r, p3, p4, then 1 / lambda_l, 1 / lambda_r for the GPU's filtered step. Only n >= 20 (n p >= 10) takes BTPE.
void btpe_setup(uint64_t n_u, double* row) {
    const double p = 0.5, q = 1.0 - p;
    const double n = (double)n_u;
    const double np = n * p;
    const double npq = np * q;
    const double f_m = np + p;
    const int64_t m = (int64_t)f_m;
    const double p1 = std::floor(2.195 * std::sqrt(npq) - 4.6 * q) + 0.5;
    const double x_m = (double)m + 0.5;
    const double x_l = x_m - p1;
    const double x_r = x_m + p1;
    const double c = 0.134 + 20.5 / (15.3 + (double)m);
    const double p2 = p1 * (1. + 2. * c);
    const double al = (f_m - x_l) / (f_m - x_l * p);
    const double lambda_l = al * (1. + 0.5 * al);
    const double ar = (x_r - f_m) / (x_r * q);
    const double lambda_r = ar * (1. + 0.5 * ar);
    const double p3 = p2 + c / lambda_l;
    const double p4 = p3 + c / lambda_r;
    // (+ 1 / lambda_l, 1 / lambda_r: not the reference's arithmetic; only the GPU's filtered region-3/4 step uses them,
    // refdraws::trunc_log_ratio, where a quotient within ~2^-37 decides)
    const double v[14] = {npq, (double)m, p1, x_m, x_l, x_r, c, p2, lambda_l, lambda_r, p3, p4, 1.0 / lambda_l, 1.0 / lambda_r};
    for (int i = 0; i < 14; ++i) row[i] = v[i];
}
constexpr int kBtpeRow = 16;  // refdraws::kBtpeRow

// A chunk as planned (first, n, its grid, rotation's partition size, the drain control), and what the context adds.
struct Chunk : ecdna::plan::ChunkPlan {
    std::vector<hipEvent_t> ev;  // per growth phase (one in an ordinary run): start, stepper done, passes done
    std::vector<ecdna::RotPart> rot_init;  // replicate rotation (rot_n_pad > 0): the counters it starts from
};

// A device buffer of the acceptance pass: it belongs to the context but not to `owned`, as it is allocated at the first
// ecdna_ssa_ctx_accept that needs it and replaced by a larger one when a later call needs more.
struct AcceptBuf {
    void* ptr = nullptr;
    uint64_t bytes = 0;
};

// A store of kept samples (m = 0: the context has no such block): the keep block's (ecdna_ssa_keep_t), one slice, or the
// timepoint keep block's (ecdna_ssa_keep_timepoints_t), a slice per timepoint — the run's snapshots or growth phases.
// Headers [T][n] and cells [T][n][m] are sized by the run and written by the keep pass of every chunk. The store's last
// rescore left its records [T][P][n] with the targets' CDFs [T][P][bins] and scalars [T][P][3] (and their host copies,
// which an asynchronous upload reads) in buffers that belong to the context as the acceptance pass's do. The pooled
// histogram and the gather's index and staging are the context's, shared by its stores (both calls are synchronous).
struct KeptStore {
    uint32_t m = 0, T = 0;
    uint2* d_headers = nullptr;
    uint16_t* d_cells = nullptr;
    AcceptBuf stats, cdf, scalars;
    std::vector<double> host_cdf, host_scalars;
    bool valid = false;    // (a launch invalidates the records)
    bool pending = false;  // a rescore was enqueued since the stream was last drained
    uint32_t targets = 0;  // the P of the last rescore: targets per slice (the timepoint keep block: 1)
    hipStream_t stream = nullptr;
};

}  // namespace

struct ecdna_ssa_ctx {
    ecdna_ssa_params_t p{};
    int device = 0;
    int cus = 0;
    uint64_t row_stride = 0;  // device rows (the bin store: its large-k rows, big_cap cells)
    uint64_t out_stride = 0;  // downloaded and snapshot rows (cell_cap cells)
    uint32_t big_cap = 0;     // bin store: large-k row capacity
    uint64_t chunk_reps = 0;
    uint32_t stepper_blocks_cap = 0;
    int window = 1;  // LDS tail window stepper (ECDNA_SSA_WINDOW=0 selects the HBM-only variant)
    // bin store (ECDNA_FLAG_BIN_STORE): binned copy numbers (0 = row store), u32 counters, the
    // per-replicate final counters [chunk_reps][bin_k]
    uint32_t bin_k = 0;
    int bin_c32 = 0;
    uint64_t bag_bytes = 0;  // bytes of one replicate's bin counters
    int bin_ilp = 0;  // the bin stepper's schedule: 0 default, 1 max-ILP (lone waves), 2 128-VGPR K = 64, 3 max-ILP paired lanes (ssa_launch.h)
    unsigned char* d_bags = nullptr;
    uint32_t stepper_block = ecdna::kStepperBlock;
    // reference draws (ECDNA_FLAG_REFERENCE_DRAWS): the ChaCha8 key and the BTPE constants per copy number
    bool refdraws = false;
    uint32_t* d_ref_key = nullptr;
    double* d_ref_btpe = nullptr;
    uint64_t* d_rng_words = nullptr;  // [n] ChaCha8 stream position of each replicate at its end
    // owned copies of the host inputs
    std::vector<ecdna_rates_t> rates;
    std::vector<uint16_t> init_copies;
    std::vector<uint32_t> init_offsets;
    std::vector<uint64_t> init_nminus_set;
    std::vector<uint64_t> snap_cells;
    // ABC statistics target
    ecdna::StatsTarget target{};  // (cdf: d_target_cdf)
    double* d_target_cdf = nullptr;
    ecdna_rep_stats_t* d_stats = nullptr;
    // end-of-run subsampling (subsample_cells > 0): the samples' statistics [n] and histogram [n_sets][bins]
    ecdna_rep_stats_t* d_sample_stats = nullptr;
    uint64_t* d_sample_hist = nullptr;
    // per-snapshot ABC statistics (ecdna_ssa_ext_t.snapshot_stats): statistics [n][S] and histograms [S][n_sets][bins]
    // of the saved states and (snap_m > 0) of their samples; each snapshot's target: CDF [S][bins], scalars [S][3]
    bool snap_stats = false;
    uint32_t snap_m = 0;
    bool snap_rows_local = false;  // d_snap_rows holds one chunk's rows (scratch), not the run's
    ecdna_rep_stats_t* d_snap_stats = nullptr;
    ecdna_rep_stats_t* d_snap_sample_stats = nullptr;
    uint64_t* d_snap_hist = nullptr;
    uint64_t* d_snap_sample_hist = nullptr;
    double* d_snap_target_cdf = nullptr;
    double* d_snap_target_scalars = nullptr;
    // serial passaging (ecdna_ssa_passages_t; 0 = an ordinary run): G growth phases per chunk, each started from the
    // founders the previous phase's sample left (one chunk's worth, written by ssa_passage). Every phase's outputs
    // are sized G x run; the ordinary buffers receive phase G - 1's at the end of a launch.
    uint32_t n_passages = 0;
    uint32_t passage_m = 0;
    uint64_t founder_stride = 0;
    uint16_t* d_founder_rows = nullptr;     // [chunk_reps][founder_stride]
    uint2* d_founder_counts = nullptr;      // [chunk_reps] {n-, n+}
    ecdna_rep_summary_t* d_pas_summ = nullptr;      // [G][n]
    uint64_t* d_pas_hist = nullptr;                 // [G][n_sets][bins]
    ecdna_totals_t* d_pas_tot = nullptr;            // [G][n_sets]
    ecdna_rep_stats_t* d_pas_stats = nullptr;       // [G][n]
    ecdna_rep_stats_t* d_pas_sample_stats = nullptr;// [G][n]
    uint64_t* d_pas_sample_hist = nullptr;          // [G][n_sets][bins]
    double* d_pas_target_cdf = nullptr;             // [G][bins], or nullptr: no target
    std::vector<double> pas_target_scalars;         // [G][3]: the targets' mean, entropy, N+ frequency
    // a cohort of targets (ecdna_ssa_cohort_t; 0 = none): every replicate's final state scored against each of P targets
    // (ssa_cohort.hip). Records [P][n], the samples' only with sample sizes (cohort_groups.n_groups > 0); each target's
    // CDF [P][bins] and scalars [P][3]
    uint32_t n_cohort = 0;
    ecdna::cohort::Groups cohort_groups;
    ecdna_rep_stats_t* d_coh_stats = nullptr;
    ecdna_rep_stats_t* d_coh_sample_stats = nullptr;
    double* d_coh_target_cdf = nullptr;
    double* d_coh_target_scalars = nullptr;
    // device buffers: every one is allocated by ctx_alloc / ctx_upload, which list it in `owned` for free_ctx
    // (d_hist / d_tot: the caller's output buffers or d_hist_own / d_tot_own, never owned themselves)
    std::vector<void*> owned;
    float4* d_rates = nullptr;
    uint16_t* d_init = nullptr;
    uint32_t* d_init_off = nullptr;
    uint64_t* d_init_nm = nullptr;
    uint64_t* d_snap_cells = nullptr;
    ecdna_snapshot_t* d_snap_meta = nullptr;
    uint16_t* d_snap_rows = nullptr;
    uint16_t* d_rows = nullptr;
    ecdna_rep_summary_t* d_summ = nullptr;
    uint32_t* d_heads = nullptr;  // one work counter per chunk
    uint32_t* d_order = nullptr;  // [n] chunk-local start order (set_cost_hint) or nullptr
    // replicate rotation (bin store): per-partition counters, state bytes, parked scalars (one chunk's worth)
    ecdna::RotPart* d_rot_parts = nullptr;
    uint32_t* d_rot_flags = nullptr;
    uint4* d_rot_park = nullptr;
    uint32_t rot_tick_log2 = 11;
    int32_t rot_park_min = 0;
    uint64_t* d_hist_own = nullptr;
    ecdna_totals_t* d_tot_own = nullptr;
    uint64_t* d_hist = nullptr;
    ecdna_totals_t* d_tot = nullptr;
    hipStream_t last_stream = nullptr;
    std::vector<Chunk> chunks;
    bool launched = false;
    // the acceptance pass (ecdna_ssa_ctx_accept): mask [n] u32, counts [Q][n_sets] u64, workgroup counts, and the list's
    // ids [cap] and records [cap][T]; what the last call left for ecdna_ssa_ctx_download_accept (a launch invalidates it)
    AcceptBuf acc_mask, acc_counts, acc_blocks, acc_ids, acc_list;
    bool accept_valid = false;
    uint32_t acc_rows = 0, acc_timepoints = 0, acc_list_row = 0;
    uint64_t acc_list_cap = 0;  // entries of the device list: min(list_capacity, n_replicates)
    // the select passes (ecdna_ssa_ctx_select / _select_digits): the keys [4][n] u64 of one (source, timepoint mask),
    // kept between passes and calls until a launch replaces the records they were made from, and one pass's histogram
    // [4][kMaxSelectGroups][256] u64. Allocated at the first call, freed at destroy.
    AcceptBuf sel_keys, sel_hist;
    bool sel_keys_valid = false;
    uint32_t sel_source = 0;
    uint64_t sel_tmask = 0;
    // the kept samples: the keep block's store (ecdna_ssa_ctx_rescore's records [P][n]) and the timepoint keep block's
    // (ecdna_ssa_ctx_rescore_timepoints's [T][n]), each with its own records, targets and validity; and what the passes
    // over either share: the pooled histogram [T][sets][bins], the gather's index [n_ids] and staging [T][n_ids]
    KeptStore kept, kept_tp;
    AcceptBuf pool_hist, gat_index, gat_headers, gat_cells;
    // the acceptance over repeated thinnings (ecdna_ssa_ctx_accept_draws): the call's own target CDFs [targets][bins]
    // and scalars [targets][3] (and their host copies, which an asynchronous upload reads), passes [n][Q] u8 and sums
    // [Q][n_sets] u64; what the last call left for ecdna_ssa_ctx_download_accept_draws (a launch invalidates it)
    AcceptBuf adr_cdf, adr_scalars, adr_passes, adr_sums;
    std::vector<double> adr_host_cdf, adr_host_scalars;
    bool adr_valid = false, adr_pending = false;
    uint32_t adr_rows = 0;
    hipStream_t adr_stream = nullptr;
    // the pooling over thinning draws (ecdna_ssa_ctx_pool_draws): the call's own target CDFs and scalars, and its pooled
    // arrays, thinned [targets][sets][bins] then kept [slices][sets][bins] u64. The call is synchronous and holds no result.
    AcceptBuf pdr_cdf, pdr_scalars, pdr_pool;
    // the select over thinning draws (ecdna_ssa_ctx_select_draws / _select_draws_digits): the call's own target CDFs and
    // scalars, its keys [4][n x n_draws] u64 and one pass's histogram; the block the keys were made for, kept between
    // the passes of _select_draws_digits until a launch replaces the kept samples they were made from
    AcceptBuf sdr_cdf, sdr_scalars, sdr_keys, sdr_hist;
    bool sdr_keys_valid = false;
    ecdna::select_draws::Block sdr_block;
};

namespace {

// the flags the kernels see: the caller's, plus the internal snapshot bit that selects the runtime-flags instances
// and the passage bit that selects the instances that start from founders
uint32_t kernel_flags(const ecdna_ssa_ctx& c) {
    return c.p.flags | (c.p.n_snapshots ? ecdna::kFlagSnapshotsRt : 0u) | (c.n_passages ? ecdna::kFlagPassageRt : 0u);
}

int pick_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(ECDNA_E_NODEVICE, "no HIP device");
    if (dev < 0 || dev >= n) return fail(ECDNA_E_NODEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(ECDNA_E_NODEVICE, "device query failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ECDNA_E_NODEVICE, std::string("not a gfx950 device: ") + prop.gcnArchName);
    if (hipSetDevice(dev) != hipSuccess) return fail(ECDNA_E_NODEVICE, "hipSetDevice failed");
    return ECDNA_OK;
}

void free_ctx(ecdna_ssa_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto& ch : c->chunks)
        for (auto& e : ch.ev)
            if (e) (void)hipEventDestroy(e);
    for (void* d : c->owned) (void)hipFree(d);
    for (AcceptBuf* b : {&c->acc_mask, &c->acc_counts, &c->acc_blocks, &c->acc_ids, &c->acc_list, &c->sel_keys,
                         &c->sel_hist, &c->pool_hist, &c->gat_index, &c->gat_headers, &c->gat_cells, &c->kept.stats,
                         &c->kept.cdf, &c->kept.scalars, &c->kept_tp.stats, &c->kept_tp.cdf, &c->kept_tp.scalars,
                         &c->adr_cdf, &c->adr_scalars, &c->adr_passes, &c->adr_sums, &c->pdr_cdf, &c->pdr_scalars,
                         &c->pdr_pool, &c->sdr_cdf, &c->sdr_scalars, &c->sdr_keys, &c->sdr_hist})
        if (b->ptr) (void)hipFree(b->ptr);
    delete c;
}

// A device buffer of `count` elements that the context owns from here on; ctx_upload: holding a copy of `host`
// (elements of the same size). Under TRY a failure is reported with the call's text, which names the buffer.
template <typename T>
hipError_t ctx_alloc(ecdna_ssa_ctx* c, T** ptr, uint64_t count) {
    const hipError_t e = hipMalloc(ptr, count * sizeof(T));
    if (e == hipSuccess) c->owned.push_back(*ptr);
    return e;
}
template <typename T, typename H>
hipError_t ctx_upload(ecdna_ssa_ctx* c, T** ptr, const std::vector<H>& host) {
    static_assert(sizeof(T) == sizeof(H), "ctx_upload copies bytes");
    const hipError_t e = ctx_alloc(c, ptr, host.size());
    return e != hipSuccess ? e : hipMemcpy(*ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
}
// `count` elements from the device to the host, and from device to device on a stream.
template <typename T>
hipError_t to_host(T* out, const T* dev, uint64_t count) {
    return hipMemcpy(out, dev, count * sizeof(T), hipMemcpyDeviceToHost);
}
template <typename T>
hipError_t copy_async(T* dst, const T* src, uint64_t count, hipStream_t st) {
    return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, st);
}

// The preludes of the sync and download functions: a context that was launched; its device current and its stream
// drained. (Between the two a download checks what else it needs, and returns early when there is nothing to copy.)
int ctx_launched(const ecdna_ssa_ctx* c, const char* what = "download before launch") {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched) return fail(ECDNA_E_STATE, what);
    return ECDNA_OK;
}
int ctx_drain(ecdna_ssa_ctx* c) {
    TRY(hipSetDevice(c->device));
    TRY(hipStreamSynchronize(c->last_stream));
    return ECDNA_OK;
}

// ---- ecdna_ssa_ctx_create_cohort, step by step (build_ctx has the order: the chunk size depends on what is allocated
// before gather_facts asks for the free memory) ----

// Sum of a target histogram (> 0 for a usable target), and for `count` of them ([count][bins]) what the kernels
// compare against: the CDFs over the bins ([count][bins]) and the scalars ([count][3]: mean, entropy, N+ frequency;
// the overflow bin counts at k = bins - 1).
double target_total(const uint64_t* hist, uint32_t bins) {
    double tot = 0.0;
    for (uint32_t b = 0; b < bins; ++b) tot += (double)hist[b];
    return tot;
}
void summarize_targets(const uint64_t* hists, uint64_t count, uint32_t bins, double* out_cdf, double* out_scalars) {
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t* hist = hists + i * bins;
        const double tot = target_total(hist, bins);
        double acc = 0.0, ksum = 0.0, ent = 0.0;
        for (uint32_t b = 0; b < bins; ++b) {
            const double pb = (double)hist[b] / tot;
            acc += pb;
            out_cdf[i * bins + b] = acc;
            ksum += (double)b * (double)hist[b];
            if (pb > 0.0) ent -= pb * std::log(pb);
        }
        out_scalars[3 * i] = ksum / tot;
        out_scalars[3 * i + 1] = ent;
        out_scalars[3 * i + 2] = 1.0 - (double)hist[0] / tot;
    }
}

// The context's own copies of the caller's inputs, and what the parameters alone decide (ssa_plan.hpp run_shape):
// strides and the cell store.
ecdna::plan::RunShape adopt_params(ecdna_ssa_ctx* c, const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                   const ecdna_ssa_passages_t* pas, const ecdna::plan::Knobs& knobs) {
    c->p = *p;
    c->device = p->device;
    if (pas) {
        c->n_passages = pas->n_passages;
        c->passage_m = pas->passage_cells;
    }
    c->snap_stats = ext && ext->snapshot_stats;
    if (c->snap_stats) c->snap_m = ext->snapshot_subsample_cells;
    c->rates.assign(p->rates, p->rates + p->n_param_sets);
    uint64_t n_init = p->init_set_offsets ? p->init_set_offsets[p->n_param_sets] : p->init_nplus;
    c->init_copies.assign(p->init_copies ? p->init_copies : nullptr,
                          p->init_copies ? p->init_copies + n_init : nullptr);
    if (c->init_copies.empty()) c->init_copies.push_back(1);
    if (p->init_set_offsets) c->init_offsets.assign(p->init_set_offsets, p->init_set_offsets + p->n_param_sets + 1);
    if (p->init_set_nminus) c->init_nminus_set.assign(p->init_set_nminus, p->init_set_nminus + p->n_param_sets);
    if (p->n_snapshots) c->snap_cells.assign(p->snapshot_cells, p->snapshot_cells + p->n_snapshots);
    c->p.snapshot_cells = nullptr;
    c->p.rates = nullptr;
    c->p.init_copies = nullptr;
    c->p.init_set_offsets = nullptr;
    c->p.init_set_nminus = nullptr;
    c->p.stats_target_hist = nullptr;

    ecdna::plan::RunShape s = ecdna::plan::run_shape(*p, c->snap_stats, c->n_passages, c->passage_m, knobs);
    s.stepper_block = s.refdraws ? (uint32_t)ecdna::refdraws_block()
                      : s.bin_k  ? (uint32_t)ecdna::bin_stepper_block(s.bin_k)
                                 : (uint32_t)ecdna::kStepperBlock;
    c->refdraws = s.refdraws;
    c->founder_stride = s.founder_stride;
    c->row_stride = s.row_stride;
    c->out_stride = s.out_stride;
    c->big_cap = s.big_cap;
    c->bin_k = s.bin_k;
    c->bin_c32 = s.bin_c32;
    c->bag_bytes = s.bag_bytes;
    c->stepper_block = s.stepper_block;
    c->snap_rows_local = s.snap_rows_local;
    return s;
}

int upload_inputs(ecdna_ssa_ctx* c) {
    hipDeviceProp_t prop;
    TRY(hipGetDeviceProperties(&prop, c->device));
    c->cus = prop.multiProcessorCount;
    std::vector<float4> r4(c->rates.size());
    for (size_t s = 0; s < r4.size(); ++s) r4[s] = make_float4(c->rates[s].b0, c->rates[s].b1, c->rates[s].d0, c->rates[s].d1);
    TRY(ctx_upload(c, &c->d_rates, r4));
    TRY(ctx_upload(c, &c->d_init, c->init_copies));
    if (!c->init_offsets.empty()) TRY(ctx_upload(c, &c->d_init_off, c->init_offsets));
    if (!c->init_nminus_set.empty()) TRY(ctx_upload(c, &c->d_init_nm, c->init_nminus_set));
    if (!c->snap_cells.empty()) TRY(ctx_upload(c, &c->d_snap_cells, c->snap_cells));
    return ECDNA_OK;
}

// ABC statistics: the statistics themselves, and each target's CDF over the bins and its mean / entropy / N+ frequency
// (the overflow bin counts at k = bins - 1), computed once on the host: the run's, each phase's, each snapshot's.
int upload_targets(ecdna_ssa_ctx* c, const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                   const ecdna_ssa_passages_t* pas) {
    const uint32_t bins = p->hist_bins;
    if ((p->flags & ECDNA_FLAG_REP_STATS) && p->n_replicates) {
        TRY(ctx_alloc(c, &c->d_stats, p->n_replicates));
        if (p->stats_target_hist) {
            if (!(target_total(p->stats_target_hist, bins) > 0.0)) return fail(ECDNA_E_INVALID, "stats_target_hist is empty");
            std::vector<double> cdf(bins);
            double sc[3];
            summarize_targets(p->stats_target_hist, 1, bins, cdf.data(), sc);
            c->target = ecdna::StatsTarget{nullptr, sc[0], sc[1], sc[2], 1u};
            TRY(ctx_upload(c, &c->d_target_cdf, cdf));
            c->target.cdf = c->d_target_cdf;
        }
    }
    if (pas && pas->passage_target_hists) {  // phase g's own target
        std::vector<double> cdf((uint64_t)pas->n_passages * bins);
        c->pas_target_scalars.assign(pas->n_passages * 3, 0.0);
        summarize_targets(pas->passage_target_hists, pas->n_passages, bins, cdf.data(), c->pas_target_scalars.data());
        TRY(ctx_upload(c, &c->d_pas_target_cdf, cdf));
    }
    if (c->snap_stats && ext->snapshot_target_hists) {
        std::vector<double> cdf((uint64_t)p->n_snapshots * bins), scal(p->n_snapshots * 3);
        summarize_targets(ext->snapshot_target_hists, p->n_snapshots, bins, cdf.data(), scal.data());
        TRY(ctx_upload(c, &c->d_snap_target_cdf, cdf));
        TRY(ctx_upload(c, &c->d_snap_target_scalars, scal));
    }
    return ECDNA_OK;
}

// The cohort block: the targets' CDFs and scalars, the grouping by sample size, and the records, sized by the run.
int adopt_cohort(ecdna_ssa_ctx* c, const ecdna_ssa_params_t* p, const ecdna_ssa_cohort_t* co) {
    const uint32_t bins = p->hist_bins, P = co->n_targets;
    c->n_cohort = P;
    c->cohort_groups = ecdna::cohort::group_by_sample_size(co->sample_cells, P);
    std::vector<double> cdf((uint64_t)P * bins), scal(P * 3);
    summarize_targets(co->target_hists, P, bins, cdf.data(), scal.data());
    TRY(ctx_upload(c, &c->d_coh_target_cdf, cdf));
    TRY(ctx_upload(c, &c->d_coh_target_scalars, scal));
    const uint64_t records = (uint64_t)P * std::max<uint64_t>(p->n_replicates, 1);
    // (the samples' records only with sample sizes)
    for (ecdna_rep_stats_t** buf : {&c->d_coh_stats, c->cohort_groups.n_groups ? &c->d_coh_sample_stats : nullptr}) {
        if (!buf) continue;
        const hipError_t e = ctx_alloc(c, buf, records);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP,
                        "ecdna_ssa_ctx_create_cohort: the cohort records (" +
                            std::to_string(records * sizeof(ecdna_rep_stats_t)) + " bytes) do not fit: " +
                            hipGetErrorString(e));
        }
    }
    return ECDNA_OK;
}

// A keep block's store of T slices of samples of m cells: the headers [T][n] and cells [T][n][m], sized by the run.
// `who`: the create call of the block, for the message.
int adopt_kept_store(ecdna_ssa_ctx* c, KeptStore* s, uint32_t T, uint32_t m, const char* who) {
    s->T = T;
    s->m = m;
    const uint64_t n1 = std::max<uint64_t>(c->p.n_replicates, 1);
    hipError_t e = ctx_alloc(c, &s->d_headers, T * n1);
    if (e == hipSuccess) e = ctx_alloc(c, &s->d_cells, T * n1 * m);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP,
                    std::string(who) + ": the kept samples (" + std::to_string(ecdna::keep::bytes(T, n1, m)) +
                        " bytes) do not fit: " + hipGetErrorString(e));
    }
    return ECDNA_OK;
}

// Outputs sized by the run (not by the chunk).
int alloc_outputs(ecdna_ssa_ctx* c) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n = p.n_replicates, n1 = std::max<uint64_t>(n, 1);
    const uint64_t nb = (uint64_t)p.n_param_sets * p.hist_bins;
    if (p.subsample_cells || c->n_passages) {  // (a passage run: the last phase's sample)
        TRY(ctx_alloc(c, &c->d_sample_stats, n1));
        TRY(ctx_alloc(c, &c->d_sample_hist, nb));
    }
    if (c->n_passages) {  // every phase's outputs, sized G x run; the last phase's are copied into the ordinary buffers
        const uint64_t G = c->n_passages;
        TRY(ctx_alloc(c, &c->d_pas_summ, G * n1));
        TRY(ctx_alloc(c, &c->d_pas_stats, G * n1));
        TRY(ctx_alloc(c, &c->d_pas_sample_stats, G * n1));
        TRY(ctx_alloc(c, &c->d_pas_hist, G * nb));
        TRY(ctx_alloc(c, &c->d_pas_sample_hist, G * nb));
        TRY(ctx_alloc(c, &c->d_pas_tot, G * p.n_param_sets));
    }
    // per-snapshot statistics: sized by the run (the snapshot rows they are computed from may be one chunk's)
    if (c->snap_stats) {
        const uint64_t S = p.n_snapshots;
        TRY(ctx_alloc(c, &c->d_snap_stats, n1 * S));
        TRY(ctx_alloc(c, &c->d_snap_hist, S * nb));
        if (c->snap_m) {
            TRY(ctx_alloc(c, &c->d_snap_sample_stats, n1 * S));
            TRY(ctx_alloc(c, &c->d_snap_sample_hist, S * nb));
        }
    }
    TRY(ctx_alloc(c, &c->d_hist_own, nb));
    TRY(ctx_alloc(c, &c->d_tot_own, p.n_param_sets));
    TRY(hipMemset(c->d_hist_own, 0, nb * sizeof(uint64_t)));
    TRY(hipMemset(c->d_tot_own, 0, p.n_param_sets * sizeof(ecdna_totals_t)));
    c->d_hist = c->d_hist_own;
    c->d_tot = c->d_tot_own;
    TRY(ctx_alloc(c, &c->d_summ, n1));
    if (p.n_snapshots && n) {  // snapshot outputs cover the whole run (not chunked)
        TRY(ctx_alloc(c, &c->d_snap_meta, n * p.n_snapshots));
        if (p.flags & ECDNA_FLAG_SNAPSHOT_ROWS) TRY(ctx_alloc(c, &c->d_snap_rows, n * p.n_snapshots * c->out_stride));
    }
    return ECDNA_OK;
}

// The kernel a context of this shape launches under the row store's window variant / the bin stepper's schedule
// (nullptr: the shape has no such instance), for the occupancy queries and ecdna_ssa_ctx_instance.
const void* stepper_fn(const ecdna_ssa_ctx& c, int window, int schedule) {
    const ecdna_ssa_params_t& p = c.p;
    if (c.refdraws) return ecdna::refdraws_kernel(p.process, p.segregation);
    if (c.bin_k) return ecdna::bin_stepper_kernel(p.process, p.segregation, c.bin_k, c.bin_c32, kernel_flags(c), schedule);
    return ecdna::stepper_kernel(p.process, p.segregation, window, kernel_flags(c));
}

// What the planner asks of the runtime. The free memory is read here: after the run-sized outputs are allocated,
// before the chunk's buffers.
int gather_facts(const ecdna_ssa_ctx* c, const ecdna::plan::Knobs& knobs, ecdna::plan::DeviceFacts* f) {
    f->cus = c->cus;
    size_t free_b = 0, total_b = 0;
    TRY(hipMemGetInfo(&free_b, &total_b));
    f->free_bytes = free_b;
    if (hipDeviceGetAttribute(&f->xccs, hipDeviceAttributeNumberOfXccs, c->device) != hipSuccess) f->xccs = 0;
    const int block = (int)c->stepper_block, window = knobs[ecdna::plan::WINDOW] ? 1 : 0;
    if (c->refdraws) {
        TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&f->occ_refdraws, stepper_fn(*c, window, 0), block, 0));
    } else if (c->bin_k) {
        // every instance of the shape (a schedule without an instance of its own launches the default's)
        for (int s = 0; s < 4; ++s) {
            const void* fn = stepper_fn(*c, window, s);
            if (fn && (s == 0 || fn != stepper_fn(*c, window, 0)))
                TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&f->occ_bins[s], fn, block, 0));
        }
    } else {
        TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&f->occ_rows, stepper_fn(*c, window, 0), block, 0));
    }
    return ECDNA_OK;
}

// The chunk's buffers, the chunks with their events and start order, and the buffers of what the plan turned on.
int alloc_plan(ecdna_ssa_ctx* c, const ecdna::plan::LaunchPlan& pl, const float* set_cost_hint) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n = p.n_replicates;
    if (pl.chunk_reps == 0) return fail(ECDNA_E_NOMEM, "one replicate row does not fit in device memory");
    c->chunk_reps = pl.chunk_reps;
    c->window = pl.window;
    c->bin_ilp = pl.schedule;
    c->stepper_blocks_cap = pl.stepper_blocks_cap;
    c->rot_tick_log2 = pl.rot_tick_log2;
    c->rot_park_min = pl.rot_park_min;
    TRY(ctx_alloc(c, &c->d_rows, c->chunk_reps * c->row_stride));
    if (c->bin_k) TRY(ctx_alloc(c, &c->d_bags, c->chunk_reps * c->bag_bytes));
    if (c->snap_rows_local) TRY(ctx_alloc(c, &c->d_snap_rows, c->chunk_reps * p.n_snapshots * c->out_stride));
    if (c->n_passages) {
        TRY(ctx_alloc(c, &c->d_founder_rows, c->chunk_reps * c->founder_stride));
        TRY(ctx_alloc(c, &c->d_founder_counts, c->chunk_reps));
    }

    TRY(ctx_alloc(c, &c->d_heads, std::max<uint64_t>(pl.chunks.size(), 1)));
    for (const ecdna::plan::ChunkPlan& cp : pl.chunks) {
        c->chunks.emplace_back();
        Chunk& ch = c->chunks.back();
        static_cast<ecdna::plan::ChunkPlan&>(ch) = cp;
        ch.ev.assign(3u * std::max<uint32_t>(c->n_passages, 1u), nullptr);
        for (auto& e : ch.ev) TRY(hipEventCreate(&e));
        if (ch.rot_n_pad) {
            ch.rot_init.assign(ecdna::kRotParts, ecdna::RotPart{});
            for (uint32_t x = 0; x < ecdna::kRotParts; ++x)
                ch.rot_init[x].waiting = ch.rot_init[x].fresh = ecdna::plan::rot_part_count(ch.n, x);
        }
    }

    // start order (set_cost_hint): within each chunk, replicates of costlier sets first, then by id
    if (set_cost_hint && n) {
        const uint64_t stride = rid_stride(p);
        std::vector<uint32_t> order(n);
        for (const Chunk& ch : c->chunks) {
            uint32_t* o = order.data() + ch.first;
            for (uint32_t i = 0; i < ch.n; ++i) o[i] = i;
            auto cost = [&](uint32_t i) {
                const float v = set_cost_hint[(p.first_replicate + (ch.first + i) * stride) / p.reps_per_set];
                return v == v ? v : 0.0f;  // (NaN: no preference)
            };
            std::stable_sort(o, o + ch.n, [&](uint32_t x, uint32_t y) { return cost(x) > cost(y); });
        }
        TRY(ctx_upload(c, &c->d_order, order));
    }

    if (c->refdraws) {
        std::vector<uint32_t> key(8);
        chacha_key_from_u64(p.seed, key.data());
        TRY(ctx_upload(c, &c->d_ref_key, key));
        std::vector<double> bt((uint64_t)32768 * kBtpeRow, 0.0);
        for (uint64_t k = 10; k < 32768; ++k) btpe_setup(2 * k, bt.data() + k * kBtpeRow);
        TRY(ctx_upload(c, &c->d_ref_btpe, bt));
        TRY(ctx_alloc(c, &c->d_rng_words, std::max<uint64_t>(n, 1)));
    }
    if (pl.any_rotation) {
        TRY(ctx_alloc(c, &c->d_rot_parts, ecdna::kRotParts));
        TRY(ctx_alloc(c, &c->d_rot_flags, ecdna::kRotParts * pl.rot_n_pad_max));
        TRY(ctx_alloc(c, &c->d_rot_park, c->chunk_reps * ecdna::kParkVecs));
    }
    return ECDNA_OK;
}

// Gather, plan, allocate: what the run's shape and the device say, the plan they give (ssa_plan.hpp: every launch
// decision of create), and the buffers the plan asks for.
int build_ctx(ecdna_ssa_ctx* c, const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
              const ecdna_ssa_passages_t* pas, const ecdna_ssa_cohort_t* co, const ecdna_ssa_keep_t* keep,
              const ecdna_ssa_keep_timepoints_t* kt) {
    const ecdna::plan::Knobs knobs = ecdna::plan::knobs_from_env();
    const ecdna::plan::RunShape shape = adopt_params(c, p, ext, pas, knobs);
    TRY(upload_inputs(c));
    TRY(upload_targets(c, p, ext, pas));
    if (co) TRY(adopt_cohort(c, p, co));
    if (keep) TRY(adopt_kept_store(c, &c->kept, 1u, keep->keep_cells, "ecdna_ssa_ctx_create_keep"));
    if (kt)
        TRY(adopt_kept_store(c, &c->kept_tp, ecdna::keep_timepoints::timepoints(*p, ext, pas), kt->keep_cells,
                             "ecdna_ssa_ctx_create_keep_timepoints"));
    TRY(alloc_outputs(c));
    ecdna::plan::DeviceFacts facts;
    TRY(gather_facts(c, knobs, &facts));
    TRY(alloc_plan(c, ecdna::plan::plan_launch(shape, facts, knobs), p->set_cost_hint));
    return ECDNA_OK;
}

// ---- ecdna_ssa_ctx_launch, piece by piece: per chunk k and growth phase g (one in an ordinary run) the stepper, the
// histogram pass and the sampling passes the run asks for, in this order on the stream ----

ecdna::StepperArgs stepper_args(const ecdna_ssa_ctx* c, const Chunk& ch, size_t k, uint32_t g) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n_run = std::max<uint64_t>(p.n_replicates, 1);
    ecdna::StepperArgs a{};
    a.rows = c->d_rows;
    a.summaries = (c->n_passages ? c->d_pas_summ + g * n_run : c->d_summ) + ch.first;
    a.head = c->d_heads + k;
    a.order = c->d_order ? c->d_order + ch.first : nullptr;
    a.rates = c->d_rates;
    a.init_copies = c->d_init;
    a.init_offsets = c->d_init_off;
    a.init_nminus_set = c->d_init_nm;
    a.row_stride = c->row_stride;
    a.seed = passage_seed(p.seed, g);  // (an ordinary run: the seed)
    if (g > 0) {  // started from the founders the previous phase's sample left
        a.founder_rows = c->d_founder_rows;
        a.founder_counts = c->d_founder_counts;
        a.founder_stride = c->founder_stride;
    }
    a.rid_stride = rid_stride(p);
    a.rid0 = p.first_replicate + ch.first * a.rid_stride;
    a.reps_per_set = p.reps_per_set;
    a.max_cells = p.max_cells;
    a.init_nminus = p.init_nminus;
    a.max_time = p.max_time;
    a.max_time32 = (float)p.max_time;
    a.n = ch.n;
    a.init_nplus = p.init_nplus;
    a.max_iter = (uint32_t)p.max_iter;
    a.cell_cap = p.cell_cap;
    a.flags = kernel_flags(*c);  // (with the internal bits: they select the kernel instance)
    // (n- + n+) * 2 >= max_cells  <=>  n- + n+ >= ceil(max_cells / 2)
    a.stop_cells = (p.process == ECDNA_BIRTH_DEATH && (p.flags & ECDNA_FLAG_BD_CAP_COMPAT))
                       ? p.max_cells / 2 + (p.max_cells & 1)
                       : p.max_cells;
    // (populations are u32 in every stepper: a larger bound acts as 2^32 - 1, include/ecdna_ssa.h)
    a.stop_cells = std::min<uint64_t>(a.stop_cells, 0xffffffffull);
    a.n_snap = p.n_snapshots;
    a.snap_cells = c->d_snap_cells;
    a.snap_meta = c->d_snap_meta ? c->d_snap_meta + ch.first * p.n_snapshots : nullptr;
    // (the run's rows at the chunk's offset, or the chunk's scratch)
    a.snap_rows = c->d_snap_rows;
    if (a.snap_rows && !c->snap_rows_local) a.snap_rows += ch.first * p.n_snapshots * c->out_stride;
    a.snap_stride = c->out_stride;
    a.big_cap = c->big_cap;
    a.bags = c->d_bags;
    a.admit_slot = ch.admit_slot;  // (drain control, decided at create)
    a.admit_remaining = ch.admit_remaining;
    if (ch.rot_n_pad) {  // rotation replaces the drain control
        a.rot_parts = c->d_rot_parts;
        a.rot_flags = c->d_rot_flags;
        a.rot_park = c->d_rot_park;
        a.rot_n_pad = ch.rot_n_pad;
        a.rot_tick_log2 = c->rot_tick_log2;
        a.rot_park_min = c->rot_park_min;
    }
    a.ref_key = c->d_ref_key;
    a.ref_btpe = c->d_ref_btpe;
    a.rng_words = c->d_rng_words ? c->d_rng_words + ch.first : nullptr;
    return a;
}

// The rotation state of a chunk, as every stepper launch finds it: all its replicates fresh, the padding done.
int reset_rotation(const ecdna_ssa_ctx* c, const Chunk& ch, hipStream_t st) {
    const uint64_t n_flags = (uint64_t)ecdna::kRotParts * ch.rot_n_pad;
    TRY(hipMemsetD32Async(c->d_rot_flags, ecdna::ROT_FRESH, ch.n, st));
    if (n_flags > ch.n) TRY(hipMemsetD32Async(c->d_rot_flags + ch.n, ecdna::ROT_DONE, n_flags - ch.n, st));
    TRY(hipMemcpyAsync(c->d_rot_parts, ch.rot_init.data(), ecdna::kRotParts * sizeof(ecdna::RotPart),
                       hipMemcpyHostToDevice, st));
    return ECDNA_OK;
}

// The target phase g is scored against: its own (a passage run with passage_target_hists), else the run's.
ecdna::StatsTarget phase_target(const ecdna_ssa_ctx* c, uint32_t g) {
    if (!c->n_passages || !c->d_pas_target_cdf) return c->target;
    const double* sc = c->pas_target_scalars.data() + 3 * g;
    return {c->d_pas_target_cdf + (uint64_t)g * c->p.hist_bins, sc[0], sc[1], sc[2], 1u};
}

// A workgroup's share of the chunk's n replicates in an end-of-run pass: the chunk over eight workgroups per CU, at
// least `floor`. (Eight per CU for either histogram pass: one per CU made the bin store's lane-per-replicate pass no
// faster at C3, 0.29 -> 0.30 ms, and C4's 1,024 sets 5 -> 28 ms, each workgroup walking more sets. The sampling
// passes run one wave per population: at least one per wave of the workgroup, at most the histogram pass's share,
// which bounds the sets a workgroup walks.)
uint32_t pass_reps_per_block(const ecdna_ssa_ctx* c, uint32_t n, uint32_t floor) {
    const uint32_t hist_blocks_max = (uint32_t)c->cus * 8u;
    return std::max<uint32_t>(floor, (n + hist_blocks_max - 1) / hist_blocks_max);
}
uint32_t pass_blocks(const ecdna::ChunkIds& ids) { return (ids.n + ids.reps_per_block - 1) / ids.reps_per_block; }
// The share of a pass that sums histograms per parameter set, in workgroups of `block` lanes (the histogram pass, and
// the pooling of the kept samples): at least one replicate per lane of a workgroup, or the chunk's replicates of one
// parameter set if fewer: small runs otherwise spread over 2,048 workgroups of mostly idle waves, each adding its own
// nonzero bins to the same global words (C2: 0.061 -> 0.023 ms per launch at 256, 0.038 at 64, 0.052 at 1,024;
// profiles/r06ak_hist_rpb.txt); sweeps of small sets keep about one set per workgroup
uint32_t hist_reps_per_block(const ecdna_ssa_ctx* c, uint32_t n, uint32_t block) {
    const uint64_t set_local = c->p.reps_per_set / rid_stride(c->p);
    return pass_reps_per_block(c, n, (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(block, set_local)));
}

ecdna::HistArgs hist_args(const ecdna_ssa_ctx* c, const Chunk& ch, uint32_t g, const ecdna::FinalState& fs,
                          ecdna::ChunkIds ids, const ecdna::StatsTarget& target) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t nb = (uint64_t)p.n_param_sets * p.hist_bins, n_run = std::max<uint64_t>(p.n_replicates, 1);
    const bool pas = c->n_passages != 0;
    ecdna::HistArgs h{};
    h.rows = fs.rows;
    h.summaries = fs.summaries;
    h.row_stride = fs.row_stride;
    h.bags = fs.bags;
    h.bag_k = fs.bag_k;
    h.bag_c32 = fs.bag_c32;
    h.hist = pas ? c->d_pas_hist + g * nb : c->d_hist;
    h.totals = reinterpret_cast<unsigned long long*>(pas ? c->d_pas_tot + (uint64_t)g * p.n_param_sets : c->d_tot);
    ids.reps_per_block = hist_reps_per_block(c, ch.n, ecdna::kHistBlock);
    h.ids = ids;
    h.stats = pas ? c->d_pas_stats + g * n_run + ch.first : (c->d_stats ? c->d_stats + ch.first : nullptr);
    h.target = target;
    return h;
}

// the samples' statistics and histogram, from the same final state
int launch_subsample_pass(const ecdna_ssa_ctx* c, const Chunk& ch, const ecdna::FinalState& fs, ecdna::ChunkIds ids,
                          const ecdna::StatsTarget& target, hipStream_t st) {
    ecdna::SubsampleArgs sa{};
    sa.state = fs;
    sa.target = target;
    sa.stats = c->d_sample_stats + ch.first;
    sa.sample_hist = c->d_sample_hist;
    sa.seed = c->p.seed;
    sa.m = c->p.subsample_cells;
    sa.table_slots = ecdna::subsample_table_slots(sa.m);
    ids.reps_per_block =
        pass_reps_per_block(c, ch.n, ecdna::subsample_waves(ids.bins, fs.bag_k, sa.table_slots, nullptr));
    sa.ids = ids;
    TRY(ecdna::launch_subsample(sa, pass_blocks(ids), st));
    return ECDNA_OK;
}

// the final state against every target of the cohort, and its samples against theirs
int launch_cohort_pass(const ecdna_ssa_ctx* c, const Chunk& ch, const ecdna::FinalState& fs, ecdna::ChunkIds ids,
                       hipStream_t st) {
    const ecdna::cohort::Groups& g = c->cohort_groups;
    const ecdna::cohort::LdsPlan lp = ecdna::cohort::lds_plan(ids.bins, fs.bag_k, g.max_m);
    ecdna::CohortArgs ca{};
    ca.state = fs;
    ca.stats = c->d_coh_stats + ch.first;
    ca.sample_stats = c->d_coh_sample_stats ? c->d_coh_sample_stats + ch.first : nullptr;
    ca.out_stride = std::max<uint64_t>(c->p.n_replicates, 1);
    ca.target_cdf = c->d_coh_target_cdf;
    ca.target_scalars = c->d_coh_target_scalars;
    ca.seed = c->p.seed;
    ca.n_targets = c->n_cohort;
    ca.n_groups = g.n_groups;
    ca.table_slots = lp.table_slots;
    ca.scratch_words = lp.scratch_words;
    std::copy(std::begin(g.m), std::end(g.m), ca.group_m);
    std::copy(std::begin(g.offset), std::end(g.offset), ca.group_offset);
    std::copy(std::begin(g.targets), std::end(g.targets), ca.group_targets);
    ids.reps_per_block = pass_reps_per_block(c, ch.n, lp.waves);
    ca.ids = ids;
    TRY(ecdna::launch_cohort(ca, pass_blocks(ids), st));
    return ECDNA_OK;
}

// What the passes of ssa_passage.hip share: the populations, and a sample of m cells of each under `seed` with the
// per-wave table and sort slots that its size asks for. keep_args: such samples into slice `slice` of a store, at the
// chunk's offset. set_share: the chunk's ids under the pass's share, `waves` populations per workgroup at least.
ecdna::PassageArgs sample_args(const ecdna::FinalState& fs, uint32_t m, uint64_t seed) {
    ecdna::PassageArgs pa{};
    pa.state = fs;
    pa.seed = seed;
    pa.m = m;
    pa.table_slots = ecdna::subsample_table_slots(m);
    pa.sort_slots = ecdna::passage_sort_slots(m);
    return pa;
}
ecdna::PassageArgs keep_args(const ecdna_ssa_ctx* c, const KeptStore& s, uint32_t slice, const Chunk& ch,
                             const ecdna::FinalState& fs, uint64_t seed) {
    const uint64_t at = slice * std::max<uint64_t>(c->p.n_replicates, 1) + ch.first;
    ecdna::PassageArgs pa = sample_args(fs, s.m, seed);
    pa.founder_rows = s.d_cells + at * s.m;
    pa.founder_counts = s.d_headers + at;
    pa.founder_stride = s.m;
    return pa;
}
void set_share(const ecdna_ssa_ctx* c, ecdna::PassageArgs* pa, ecdna::ChunkIds ids, uint32_t waves) {
    ids.reps_per_block = pass_reps_per_block(c, ids.n, waves);
    pa->ids = ids;
}

// phase g's measurement, and (but for the last phase) the founders of the next
int launch_passage_pass(const ecdna_ssa_ctx* c, const Chunk& ch, uint32_t g, const ecdna::FinalState& fs,
                        const ecdna::ChunkIds& ids, const ecdna::StatsTarget& target, uint64_t seed_g, hipStream_t st) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t nb = (uint64_t)p.n_param_sets * p.hist_bins, n_run = std::max<uint64_t>(p.n_replicates, 1);
    ecdna::PassageArgs pa = sample_args(fs, c->passage_m, seed_g);
    pa.target = target;
    pa.stats = c->d_pas_sample_stats + g * n_run + ch.first;
    pa.sample_hist = c->d_pas_sample_hist + g * nb;
    pa.founder_rows = g + 1u < c->n_passages ? c->d_founder_rows : nullptr;
    pa.founder_counts = c->d_founder_counts;
    pa.founder_stride = c->founder_stride;
    set_share(c, &pa, ids, ecdna::passage_waves(ids.bins, fs.bag_k, pa.table_slots, pa.sort_slots, nullptr));
    TRY(ecdna::launch_passage(pa, pass_blocks(pa.ids), st));
    return ECDNA_OK;
}

// the chunk's kept samples under `seed`, into slice `slice` of a store (ssa_passage's KEEP instance: neither statistics
// nor a histogram). The keep block: slice 0 under the run's seed. The timepoint keep block of a passage run: phase g's
// sample into slice g under the phase's key — the sample the passage pass measures and, but for the last phase, founds
// the next phase with.
int launch_keep_pass(const ecdna_ssa_ctx* c, const KeptStore& s, uint32_t slice, const Chunk& ch,
                     const ecdna::FinalState& fs, const ecdna::ChunkIds& ids, uint64_t seed, hipStream_t st) {
    ecdna::PassageArgs pa = keep_args(c, s, slice, ch, fs, seed);
    set_share(c, &pa, ids, ecdna::keep_waves(ids.bins, fs.bag_k, pa.table_slots, pa.sort_slots, nullptr));
    TRY(ecdna::launch_keep(pa, pass_blocks(pa.ids), st));
    return ECDNA_OK;
}

// the kept samples of the chunk's snapshots, from the rows the stepper just saved, into the timepoint keep block's store
// (ssa_passage's KEEP = 2 instance: one wave per (replicate, snapshot) pair; snapshot s goes to slice s)
int launch_keep_snapshots_pass(const ecdna_ssa_ctx* c, const Chunk& ch, const ecdna::StepperArgs& a,
                               const ecdna::ChunkIds& ids, hipStream_t st) {
    const ecdna::FinalState rows{a.snap_rows, nullptr, a.snap_stride, nullptr, 0u, 0u};
    ecdna::PassageArgs pa = keep_args(c, c->kept_tp, 0u, ch, rows, c->p.seed);
    pa.snap_meta = a.snap_meta;
    pa.slice_stride = std::max<uint64_t>(c->p.n_replicates, 1);
    pa.n_snap = c->p.n_snapshots;
    set_share(c, &pa, ids, ecdna::keep_snapshots_waves(ids.bins, pa.table_slots, pa.sort_slots, nullptr));
    TRY(ecdna::launch_keep_snapshots(pa, pass_blocks(pa.ids), st));
    return ECDNA_OK;
}

// the statistics of the chunk's snapshots, from the rows the stepper just saved
int launch_snapstats_pass(const ecdna_ssa_ctx* c, const Chunk& ch, const ecdna::StepperArgs& a, ecdna::ChunkIds ids,
                          hipStream_t st) {
    const ecdna_ssa_params_t& p = c->p;
    ecdna::SnapStatsArgs ta{};
    ta.snap_meta = a.snap_meta;
    ta.snap_rows = a.snap_rows;
    ta.stats = c->d_snap_stats + ch.first * p.n_snapshots;
    ta.sample_stats = c->d_snap_sample_stats ? c->d_snap_sample_stats + ch.first * p.n_snapshots : nullptr;
    ta.hist = c->d_snap_hist;
    ta.sample_hist = c->d_snap_sample_hist;
    ta.target_cdf = c->d_snap_target_cdf;
    ta.target_scalars = c->d_snap_target_scalars;
    ta.snap_stride = a.snap_stride;
    ta.seed = p.seed;
    ta.n_snap = p.n_snapshots;
    ta.n_sets = p.n_param_sets;
    ta.m = c->snap_m;
    ta.table_slots = c->snap_m ? ecdna::subsample_table_slots(c->snap_m) : 0u;
    ids.reps_per_block =
        pass_reps_per_block(c, ch.n, ecdna::snapstats_waves(ids.bins, ta.table_slots, nullptr, nullptr));
    ta.ids = ids;
    TRY(ecdna::launch_snapstats(ta, pass_blocks(ids), st));
    return ECDNA_OK;
}

// One growth phase of one chunk.
int launch_chunk_phase(ecdna_ssa_ctx* c, size_t k, uint32_t g, hipStream_t st) {
    const ecdna_ssa_params_t& p = c->p;
    const Chunk& ch = c->chunks[k];
    const hipEvent_t* ev = ch.ev.data() + 3u * g;
    // the chunk's work counter starts every phase at zero (the rotation state is reset below, per launch)
    if (g > 0) TRY(hipMemsetAsync(c->d_heads + k, 0, sizeof(uint32_t), st));
    const ecdna::StepperArgs a = stepper_args(c, ch, k, g);
    if (ch.rot_n_pad) TRY(reset_rotation(c, ch, st));
    TRY(hipEventRecord(ev[0], st));
    if (c->refdraws)
        TRY(ecdna::launch_refdraws(a, p.process, p.segregation, ch.blocks, st));
    else if (c->bin_k)
        TRY(ecdna::launch_bin_stepper(a, p.process, p.segregation, c->bin_k, c->bin_c32, c->bin_ilp, ch.blocks, st));
    else
        TRY(ecdna::launch_stepper(a, p.process, p.segregation, c->window, ch.blocks, st));
    TRY(hipEventRecord(ev[1], st));

    // what the passes share, filled once: the final state, the chunk's ids, the phase's target
    const ecdna::FinalState fs{c->d_rows, a.summaries, c->row_stride, c->d_bags, c->bin_k, (uint32_t)c->bin_c32};
    const ecdna::ChunkIds ids{a.rid0, a.rid_stride, a.reps_per_set, ch.n, p.hist_bins, 0u};  // (reps_per_block: per pass)
    const ecdna::StatsTarget target = phase_target(c, g);
    const ecdna::HistArgs h = hist_args(c, ch, g, fs, ids, target);
    TRY(ecdna::launch_hist(h, pass_blocks(h.ids), st));
    if (p.subsample_cells) TRY(launch_subsample_pass(c, ch, fs, ids, target, st));
    if (c->n_cohort) TRY(launch_cohort_pass(c, ch, fs, ids, st));
    if (c->kept.m) TRY(launch_keep_pass(c, c->kept, 0u, ch, fs, ids, p.seed, st));
    if (c->n_passages) TRY(launch_passage_pass(c, ch, g, fs, ids, target, a.seed, st));
    if (c->snap_stats) TRY(launch_snapstats_pass(c, ch, a, ids, st));
    // the timepoint keep block: phase g's sample, or the samples at the chunk's snapshots while their rows exist
    if (c->kept_tp.m && c->n_passages) TRY(launch_keep_pass(c, c->kept_tp, g, ch, fs, ids, a.seed, st));
    if (c->kept_tp.m && c->snap_stats) TRY(launch_keep_snapshots_pass(c, ch, a, ids, st));
    TRY(hipEventRecord(ev[2], st));
    return ECDNA_OK;
}

// ---- ecdna_ssa_ctx_accept: the source's records on the device and how they lie, then the pass's own buffers ----

// What an ecdna_accept_source_t names in this context (ssa_launch.h AcceptArgs has the strides' meaning); ECDNA_E_STATE
// under the conditions of the matching download.
// Whether a number names a source: the one predicate of ecdna_ssa_ctx_accept, select_source and ecdna_ssa_ctx_select (6
// and 7 are not sources).
bool is_accept_source(uint32_t source) {
    return source <= (uint32_t)ECDNA_ACCEPT_PASSAGE_SAMPLES || source == (uint32_t)ECDNA_ACCEPT_COHORT ||
           source == (uint32_t)ECDNA_ACCEPT_COHORT_SAMPLES || source == (uint32_t)ECDNA_ACCEPT_RESCORED ||
           source == (uint32_t)ECDNA_ACCEPT_RESCORED_TIMEPOINTS;
}
struct AcceptSource {
    const ecdna_rep_stats_t* stats = nullptr;
    const ecdna_rep_summary_t* summaries = nullptr;
    uint64_t rep_stride = 1, tp_stride = 0, err_stride = 0;
    uint32_t T = 1;
    bool has_target = false;
};
int accept_source(const ecdna_ssa_ctx* c, uint32_t source, AcceptSource* out) {
    const uint64_t n_run = std::max<uint64_t>(c->p.n_replicates, 1);
    AcceptSource s;
    s.summaries = c->d_summ;
    // (a passage run scores its phases against their own targets, or the run's)
    const bool run_target = c->target.has || (c->n_passages && c->d_pas_target_cdf);
    switch (source) {
        case ECDNA_ACCEPT_FINAL:
            if (!c->d_stats) return fail(ECDNA_E_STATE, "accept.source FINAL: statistics need ECDNA_FLAG_REP_STATS");
            s.stats = c->d_stats;
            s.has_target = run_target;
            break;
        case ECDNA_ACCEPT_SAMPLE:
            if (!c->d_sample_hist) return fail(ECDNA_E_STATE, "accept.source SAMPLE: the sample needs subsample_cells > 0");
            s.stats = c->d_sample_stats;
            s.has_target = run_target;
            break;
        case ECDNA_ACCEPT_SNAPSHOTS:
        case ECDNA_ACCEPT_SNAPSHOT_SAMPLES: {
            const bool samples = source == ECDNA_ACCEPT_SNAPSHOT_SAMPLES;
            if (!c->snap_stats)
                return fail(ECDNA_E_STATE, "accept.source SNAPSHOTS: snapshot statistics need ecdna_ssa_ext_t.snapshot_stats");
            if (samples && !c->snap_m)
                return fail(ECDNA_E_STATE, "accept.source SNAPSHOT_SAMPLES: the snapshot samples need "
                                           "ecdna_ssa_ext_t.snapshot_subsample_cells > 0");
            s.stats = samples ? c->d_snap_sample_stats : c->d_snap_stats;
            s.T = c->p.n_snapshots;
            s.rep_stride = s.T;
            s.tp_stride = 1;
            s.has_target = c->d_snap_target_cdf != nullptr;
            break;
        }
        case ECDNA_ACCEPT_PASSAGES:
        case ECDNA_ACCEPT_PASSAGE_SAMPLES:
            if (!c->n_passages)
                return fail(ECDNA_E_STATE, "accept.source PASSAGES: per-phase results need ecdna_ssa_ctx_create_passages");
            s.stats = source == ECDNA_ACCEPT_PASSAGES ? c->d_pas_stats : c->d_pas_sample_stats;
            s.summaries = c->d_pas_summ;
            s.T = c->n_passages;
            s.tp_stride = n_run;
            s.err_stride = n_run;
            s.has_target = run_target;
            break;
        case ECDNA_ACCEPT_COHORT:
        case ECDNA_ACCEPT_COHORT_SAMPLES: {
            const bool samples = source == ECDNA_ACCEPT_COHORT_SAMPLES;
            if (!c->n_cohort)
                return fail(ECDNA_E_STATE, "accept.source COHORT: the cohort records need ecdna_ssa_ctx_create_cohort");
            if (samples && !c->d_coh_sample_stats)
                return fail(ECDNA_E_STATE, "accept.source COHORT_SAMPLES: the cohort samples need "
                                           "ecdna_ssa_cohort_t.sample_cells");
            s.stats = samples ? c->d_coh_sample_stats : c->d_coh_stats;
            s.T = c->n_cohort;
            s.tp_stride = n_run;  // [P][n]; one summary per replicate, whatever the target
            s.has_target = true;
            break;
        }
        case ECDNA_ACCEPT_RESCORED:
            if (!c->kept.m)
                return fail(ECDNA_E_STATE, "accept.source RESCORED: the rescored records need ecdna_ssa_ctx_create_keep");
            if (!c->launched || !c->kept.valid)
                return fail(ECDNA_E_STATE, "accept.source RESCORED: no records before ecdna_ssa_ctx_rescore (a launch "
                                           "invalidates them)");
            s.stats = static_cast<const ecdna_rep_stats_t*>(c->kept.stats.ptr);
            s.T = c->kept.targets;
            s.tp_stride = c->p.n_replicates;  // [P][n], as the cohort's
            s.has_target = true;
            break;
        case ECDNA_ACCEPT_RESCORED_TIMEPOINTS:
            if (!c->kept_tp.m)
                return fail(ECDNA_E_STATE, "accept.source RESCORED_TIMEPOINTS: the rescored records need "
                                           "ecdna_ssa_ctx_create_keep_timepoints");
            if (!c->launched || !c->kept_tp.valid)
                return fail(ECDNA_E_STATE, "accept.source RESCORED_TIMEPOINTS: no records before "
                                           "ecdna_ssa_ctx_rescore_timepoints (a launch invalidates them)");
            s.stats = static_cast<const ecdna_rep_stats_t*>(c->kept_tp.stats.ptr);
            s.T = c->kept_tp.T;
            s.tp_stride = n_run;  // [T][n]
            if (c->n_passages) {  // the passage sources' error rule: every participating phase's own summary
                s.summaries = c->d_pas_summ;
                s.err_stride = n_run;
            }
            s.has_target = true;
            break;
        default:
            return fail(ECDNA_E_INVALID, "accept.source is not an ecdna_accept_source_t");
    }
    *out = s;
    return ECDNA_OK;
}

// At least `bytes` in `b`. A larger buffer is allocated before the old one is freed (hipFree waits for the device, so
// an earlier pass that still writes the old one has finished): a failure leaves the context as it was.
int accept_reserve(AcceptBuf* b, uint64_t bytes, const char* what, const char* who = "ecdna_ssa_ctx_accept") {
    if (bytes <= b->bytes) return ECDNA_OK;
    void* ptr = nullptr;
    const hipError_t e = hipMalloc(&ptr, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (the context stays usable)
        return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP,
                    std::string(who) + ": the " + what + " buffer (" + std::to_string(bytes) +
                        " bytes) does not fit: " + hipGetErrorString(e));
    }
    if (b->ptr) (void)hipFree(b->ptr);
    b->ptr = ptr;
    b->bytes = bytes;
    return ECDNA_OK;
}

// ---- ecdna_ssa_ctx_select / _select_digits: what both check after their own arguments, and one digit pass ----

// The source's records and the participating timepoints, under the checks and in the order of ecdna_ssa_ctx_accept.
// `who`: "select" or "select_digits", the prefix of the messages' field names.
struct SelectSource {
    AcceptSource src;
    uint64_t tmask = 0;
};
int select_source(const ecdna_ssa_ctx* c, uint32_t source, uint64_t timepoint_mask, const std::string& who,
                  SelectSource* out) {
    if (!is_accept_source(source))
        return fail(ECDNA_E_INVALID, who + ".source is not an ecdna_accept_source_t");
    if (c->p.n_replicates >= (1ull << 32)) return fail(ECDNA_E_INVALID, who + ": n_replicates must be < 2^32");
    TRY(accept_source(c, source, &out->src));
    const uint32_t T = out->src.T;
    const uint64_t all = T >= 64u ? ~0ull : (1ull << T) - 1ull;
    if (timepoint_mask & ~all)
        return fail(ECDNA_E_INVALID, who + ".timepoint_mask has bits at or above T = " + std::to_string(T));
    TRY(ctx_launched(c, (who + " before launch").c_str()));
    if (!out->src.has_target)
        return fail(ECDNA_E_STATE, who + ": the source's statistics were computed without a target (every distance is "
                                         "0: no quantile tells replicates apart)");
    out->tmask = timepoint_mask ? timepoint_mask : all;
    return ECDNA_OK;
}

// Replicates a workgroup of ssa_select_digits walks: eight rounds of its 256 lanes, so that the flush of its LDS table
// to the global histogram is shared by 2,048 keys (the C4 sweep: 2,048 workgroups per distance).
constexpr uint32_t kSelectRepsPerBlock = 8u * ecdna::kSelectBlock;

// One pass's histogram on the device: [4][kMaxSelectGroups][256] u64.
constexpr uint64_t kSelectHistWords = (uint64_t)ecdna::select::kDistances * ecdna::kMaxSelectGroups * ecdna::select::kDigits;

// One digit pass over keys [4][n] on stream st: out_hist[x][j][d], j < K, for the prefixes[x * stride + j]. d_hist: the
// device histogram, kSelectHistWords. Synchronises.
int digit_pass(const uint64_t* keys, uint32_t n, void* d_hist, uint32_t pass, uint32_t K, const uint64_t* prefixes,
               uint32_t stride, uint64_t* out_hist, hipStream_t st) {
    namespace sel = ecdna::select;
    ecdna::SelectArgs a{};
    a.keys = keys;
    a.hist = static_cast<unsigned long long*>(d_hist);
    a.n = n;
    a.pass = pass;
    a.reps_per_block = kSelectRepsPerBlock;
    uint32_t group[sel::kDistances][sel::kMaxRanks];
    for (uint32_t x = 0; x < sel::kDistances; ++x) {
        uint64_t top[sel::kMaxRanks];
        for (uint32_t j = 0; j < K; ++j) top[j] = sel::key_top(prefixes[(uint64_t)x * stride + j], pass);
        a.n_groups[x] = sel::dedup(top, K, a.prefix[x], group[x]);
    }
    TRY(hipMemsetAsync(d_hist, 0, kSelectHistWords * sizeof(uint64_t), st));
    TRY(ecdna::launch_select_digits(a, st));
    TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> dev(kSelectHistWords);
    TRY(to_host(dev.data(), static_cast<const uint64_t*>(d_hist), kSelectHistWords));
    for (uint32_t x = 0; x < sel::kDistances; ++x)
        for (uint32_t j = 0; j < K; ++j)
            std::copy_n(dev.data() + ((uint64_t)x * ecdna::kMaxSelectGroups + group[x][j]) * sel::kDigits, sel::kDigits,
                        out_hist + ((uint64_t)x * K + j) * sel::kDigits);
    return ECDNA_OK;
}

// One digit pass over the source's keys: makes them first unless the context holds those of this source and mask.
int select_pass(ecdna_ssa_ctx* c, uint32_t source, const SelectSource& s, uint32_t pass, uint32_t K,
                const uint64_t* prefixes, uint32_t stride, uint64_t* out_hist, const char* who) {
    namespace sel = ecdna::select;
    const uint64_t n = c->p.n_replicates;
    std::fill(out_hist, out_hist + (uint64_t)sel::kDistances * K * sel::kDigits, 0ull);
    if (!n) return ECDNA_OK;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    const bool cached = c->sel_keys_valid && c->sel_source == source && c->sel_tmask == s.tmask;
    if (!cached) {
        c->sel_keys_valid = false;
        TRY(accept_reserve(&c->sel_keys, sel::kDistances * n * sizeof(uint64_t), "keys", who));
    }
    TRY(accept_reserve(&c->sel_hist, kSelectHistWords * sizeof(uint64_t), "histogram", who));
    if (!cached) {
        ecdna::SelectKeyArgs k{};
        k.stats = s.src.stats;
        k.summaries = s.src.summaries;
        k.rep_stride = s.src.rep_stride;
        k.tp_stride = s.src.tp_stride;
        k.err_stride = s.src.err_stride;
        k.tmask = s.tmask;
        k.keys = static_cast<uint64_t*>(c->sel_keys.ptr);
        k.n = (uint32_t)n;
        k.T = s.src.T;
        TRY(ecdna::launch_select_keys(k, st));
        c->sel_source = source;
        c->sel_tmask = s.tmask;
        c->sel_keys_valid = true;
    }
    return digit_pass(static_cast<const uint64_t*>(c->sel_keys.ptr), (uint32_t)n, c->sel_hist.ptr, pass, K, prefixes,
                      stride, out_hist, st);
}

// ---- the passes over a store of kept samples: what a call of the keep block (one slice) and its twin of the timepoint
// keep block do after their own argument checks. Slice t of the buffers is a run of kept samples as the keep block's, so
// each is the keep block's pass once per slice, on offset pointers. `who`: the calling entry point, for the messages ----

// The sizes of a sized rescore (thinning mapping v1): target p of slice t is scored on sample_cells[t * P + p] cells of
// the kept sample, on thinning draw draws[t * P + p] (draws == nullptr: 0).
struct ThinSizes {
    const uint32_t* sample_cells;  // [T][P]
    const uint32_t* draws;         // [T][P] or nullptr
};

// The key and the stream field (thin::stream_tag) slice t of a store was drawn under, which its thinnings are drawn
// under too: the run's seed and field 0 for the keep store (the end of the run), seed_t and field 0 for phase t of a
// passage context, the run's seed and field t + 1 for snapshot t.
struct SliceStream {
    uint64_t seed;
    uint32_t field;
};
SliceStream slice_stream(const ecdna_ssa_ctx* c, const KeptStore& s, uint32_t t) {
    if (&s != &c->kept_tp) return {c->p.seed, 0u};
    if (c->n_passages) return {passage_seed(c->p.seed, t), 0u};
    return {c->p.seed, t + 1u};
}

// The thinning pass over slice t of a store (ssa_thin.hip), on the pointers rescore_store made for the slice.
int launch_thin_pass(const ecdna_ssa_ctx* c, const KeptStore& s, uint64_t t, uint32_t P, const ThinSizes& sizes,
                     ecdna::ThinArgs a, hipStream_t st) {
    namespace th = ecdna::thin;
    const ecdna_ssa_params_t& p = c->p;
    const th::Groups g = th::group_by_size_and_draw(sizes.sample_cells + t * P,
                                                    sizes.draws ? sizes.draws + t * P : nullptr, P, s.m);
    const th::LdsPlan l = th::lds_plan(p.hist_bins, g.max_mp);
    const SliceStream drawn = slice_stream(c, s, (uint32_t)t);
    a.seed = drawn.seed;
    a.rid0 = p.first_replicate;
    a.rid_stride = rid_stride(p);
    a.n_groups = g.n_groups;
    a.table_slots = l.table_slots;
    a.scratch_words = l.scratch_words;
    for (uint32_t j = 0; j < g.n_groups; ++j) {
        a.group_m[j] = g.m[j];
        a.group_tag[j] = th::stream_tag(drawn.field, g.d[j]);
    }
    std::copy_n(g.offset, ecdna::kMaxCohortTargets + 1u, a.group_offset);
    std::copy_n(g.targets, ecdna::kMaxCohortTargets, a.group_targets);
    a.reps_per_block = pass_reps_per_block(c, a.n, l.waves);
    TRY(ecdna::launch_thin(a, st));
    return ECDNA_OK;
}

// The targets' CDFs and scalars (summarize_targets) into the host copies, and their two uploads enqueued on st. The
// host copies must outlive the uploads: where they live is the caller's rule.
int upload_targets(const uint64_t* target_hists, uint64_t targets, uint32_t bins, std::vector<double>* host_cdf,
                   std::vector<double>* host_scalars, void* d_cdf, void* d_scalars, hipStream_t st) {
    host_cdf->resize(targets * bins);
    host_scalars->resize(targets * 3u);
    summarize_targets(target_hists, targets, bins, host_cdf->data(), host_scalars->data());
    TRY(hipMemcpyAsync(d_cdf, host_cdf->data(), host_cdf->size() * sizeof(double), hipMemcpyHostToDevice, st));
    TRY(hipMemcpyAsync(d_scalars, host_scalars->data(), host_scalars->size() * sizeof(double), hipMemcpyHostToDevice,
                       st));
    return ECDNA_OK;
}

// Slice t's samples against its P targets, target_hists [T][P][bins]: the store's records [T][P][n], enqueued on the
// stream of the last launch. sizes (nullptr: every target on the whole kept sample): each target on its own number of
// measured cells.
int rescore_store(ecdna_ssa_ctx* c, KeptStore* s, uint32_t P, const uint64_t* target_hists, const char* who,
                  const ThinSizes* sizes = nullptr) {
    const uint32_t bins = c->p.hist_bins;
    const uint64_t n = c->p.n_replicates, targets = (uint64_t)s->T * P;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    // an earlier rescore may still read the targets this one replaces (and its upload their host copies)
    if (s->pending) TRY(hipStreamSynchronize(s->stream));
    s->pending = false;
    s->valid = false;
    c->sel_keys_valid = false;  // (the select passes' keys may have been made from the records this call replaces)
    TRY(accept_reserve(&s->stats, std::max<uint64_t>(n, 1) * targets * sizeof(ecdna_rep_stats_t), "records", who));
    TRY(accept_reserve(&s->cdf, targets * bins * sizeof(double), "target CDFs", who));
    TRY(accept_reserve(&s->scalars, targets * 3u * sizeof(double), "target scalars", who));
    if (n) {
        TRY(upload_targets(target_hists, targets, bins, &s->host_cdf, &s->host_scalars, s->cdf.ptr, s->scalars.ptr, st));
        s->pending = true;
        s->stream = st;
        // slice t's part of the store, the same for either pass (RescoreArgs' fields, which ThinArgs repeats)
        auto slice = [&](auto a, uint64_t t) {
            a.headers = s->d_headers + t * n;
            a.cells = s->d_cells + t * n * s->m;
            a.out = static_cast<ecdna_rep_stats_t*>(s->stats.ptr) + t * P * n;
            a.target_cdf = static_cast<const double*>(s->cdf.ptr) + t * P * bins;
            a.target_scalars = static_cast<const double*>(s->scalars.ptr) + t * P * 3u;
            a.n = (uint32_t)n;
            a.m = s->m;
            a.bins = bins;
            a.n_targets = P;
            return a;
        };
        for (uint64_t t = 0; t < s->T; ++t) {
            if (sizes) {
                TRY(launch_thin_pass(c, *s, t, P, *sizes, slice(ecdna::ThinArgs{}, t), st));
                continue;
            }
            ecdna::RescoreArgs a = slice(ecdna::RescoreArgs{}, t);
            a.reps_per_block = pass_reps_per_block(c, (uint32_t)n, ecdna::rescore_waves(bins, nullptr));
            TRY(ecdna::launch_rescore(a, st));
        }
    }
    s->targets = P;
    s->valid = true;
    return ECDNA_OK;
}

int download_rescored_store(ecdna_ssa_ctx* c, const KeptStore& s, ecdna_rep_stats_t* out) {
    TRY(ctx_drain(c));
    const uint64_t records = (uint64_t)s.T * s.targets * c->p.n_replicates;
    if (out && records) TRY(to_host(out, static_cast<const ecdna_rep_stats_t*>(s.stats.ptr), records));
    return ECDNA_OK;
}

// Per slice and global parameter set, the sum of the histograms of the samples accepted under row `threshold` of the
// last accept: out_hist [T][sets][bins]. Synchronises.
int pool_store(ecdna_ssa_ctx* c, const KeptStore& s, uint32_t threshold, uint64_t* out_hist, const char* who) {
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n = p.n_replicates, nb = (uint64_t)p.n_param_sets * p.hist_bins, T = s.T;
    std::fill(out_hist, out_hist + T * nb, 0ull);
    if (!n) return ECDNA_OK;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    TRY(accept_reserve(&c->pool_hist, T * nb * sizeof(uint64_t), "histogram", who));
    TRY(hipMemsetAsync(c->pool_hist.ptr, 0, T * nb * sizeof(uint64_t), st));
    for (uint64_t t = 0; t < T; ++t) {
        ecdna::PoolAcceptedArgs a{};
        a.headers = s.d_headers + t * n;
        a.cells = s.d_cells + t * n * s.m;
        a.mask = static_cast<const uint32_t*>(c->acc_mask.ptr);
        a.hist = static_cast<unsigned long long*>(c->pool_hist.ptr) + t * nb;
        a.rid0 = p.first_replicate;
        a.rid_stride = rid_stride(p);
        a.reps_per_set = p.reps_per_set;
        a.n = (uint32_t)n;
        a.m = s.m;
        a.bins = p.hist_bins;
        a.q = threshold;
        // (the histogram pass's share: about one parameter set per workgroup in a sweep of small sets)
        a.reps_per_block = hist_reps_per_block(c, (uint32_t)n, ecdna::kPoolBlock);
        TRY(ecdna::launch_pool_accepted(a, st));
    }
    TRY(hipStreamSynchronize(st));
    TRY(to_host(out_hist, static_cast<const uint64_t*>(c->pool_hist.ptr), T * nb));
    return ECDNA_OK;
}

// The indices in the call, index [n_ids], of the replicates with the global `ids` (ids = NULL: none, the call's first
// n_ids are meant). `name`: the calling entry point without its prefix, as the messages name its arguments.
int kept_index(const ecdna_ssa_ctx* c, const std::string& name, uint64_t n_ids, const uint64_t* ids, uint32_t* index) {
    const ecdna_ssa_params_t& p = c->p;
    if (!ids && n_ids > p.n_replicates)
        return fail(ECDNA_E_INVALID, name + ".n_ids must be <= n_replicates when ids is NULL");
    for (uint64_t j = 0; ids && j < n_ids; ++j) {
        uint64_t i = 0;
        if (!ecdna::keep::index_of(ids[j], p.first_replicate, rid_stride(p), p.n_replicates, &i))
            return fail(ECDNA_E_INVALID, name + ".ids[" + std::to_string(j) + "] = " + std::to_string(ids[j]) +
                                             " is not a replicate of this call");
        index[j] = (uint32_t)i;
    }
    return ECDNA_OK;
}

// Every slice's samples of the replicates at `index` (kept_index), gathered on the device in that order, slice by slice,
// then copied once; index = NULL: the first n_ids samples of every slice. out_headers [T][n_ids], out_cells [T][n_ids][m].
int download_kept_store(ecdna_ssa_ctx* c, const KeptStore& s, uint64_t n_ids, const uint32_t* index,
                        ecdna_kept_t* out_headers, uint16_t* out_cells, const char* who) {
    static_assert(sizeof(ecdna_kept_t) == sizeof(uint2), "a kept header is two u32 words");
    if (!n_ids || (!out_headers && !out_cells)) return ECDNA_OK;
    TRY(ctx_drain(c));
    const uint64_t n = c->p.n_replicates, m = s.m, T = s.T;
    if (index) {
        TRY(accept_reserve(&c->gat_index, n_ids * sizeof(uint32_t), "index", who));
        TRY(accept_reserve(&c->gat_headers, T * n_ids * sizeof(uint2), "headers", who));
        TRY(accept_reserve(&c->gat_cells, T * n_ids * m * sizeof(uint16_t), "cells", who));
        hipStream_t st = c->last_stream;
        TRY(hipMemcpy(c->gat_index.ptr, index, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice));
        for (uint64_t t = 0; t < T; ++t) {
            ecdna::KeptGatherArgs a{};
            a.headers = s.d_headers + t * n;
            a.cells = s.d_cells + t * n * m;
            a.index = static_cast<const uint32_t*>(c->gat_index.ptr);
            a.out_headers = static_cast<uint2*>(c->gat_headers.ptr) + t * n_ids;
            a.out_cells = static_cast<uint16_t*>(c->gat_cells.ptr) + t * n_ids * m;
            a.n_ids = (uint32_t)n_ids;
            a.m = (uint32_t)m;
            TRY(ecdna::launch_kept_gather(a, st));
        }
        TRY(hipStreamSynchronize(st));
        if (out_headers)
            TRY(hipMemcpy(out_headers, c->gat_headers.ptr, T * n_ids * sizeof(uint2), hipMemcpyDeviceToHost));
        if (out_cells) TRY(to_host(out_cells, static_cast<const uint16_t*>(c->gat_cells.ptr), T * n_ids * m));
        return ECDNA_OK;
    }
    for (uint64_t t = 0; t < T; ++t) {
        if (out_headers)
            TRY(hipMemcpy(out_headers + t * n_ids, s.d_headers + t * n, n_ids * sizeof(uint2), hipMemcpyDeviceToHost));
        if (out_cells) TRY(to_host(out_cells + t * n_ids * m, s.d_cells + t * n * m, n_ids * m));
    }
    return ECDNA_OK;
}

const char* const kNeedsTimepoints = ": the kept timepoint samples need ecdna_ssa_ctx_create_keep_timepoints";

// ---- ecdna_ssa_ctx_accept_draws and _pool_draws: what both do with the block they share ----

// The store the block names, under the checks both calls make and in their order. name: "accept_draws" or "pool_draws",
// the prefix of the messages; invalid(keep_cells): the call's own validation (accept_draws::invalid, pool_draws::invalid).
template <class Invalid>
int draws_store(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, const std::string& name, Invalid invalid,
                KeptStore** out) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!a) return fail(ECDNA_E_INVALID, name + ": the block is NULL");
    const bool timepoints = a->timepoints == 1u;
    KeptStore* s = timepoints ? &c->kept_tp : &c->kept;
    const std::string bad = invalid(s->m ? s->m : ecdna::kMaxSubsampleCells);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    if (!s->m)
        return fail(ECDNA_E_STATE,
                    timepoints ? name + kNeedsTimepoints : name + ": the kept samples need ecdna_ssa_ctx_create_keep");
    TRY(ctx_launched(c, (name + " before launch").c_str()));
    *out = s;
    return ECDNA_OK;
}

// The part of the argument block both passes share, for the block's draws on store s: its slices and the mask are the
// plan's (accept_draws::plan), the LDS plan the call's, the targets the call's own device copies.
ecdna::DrawsArgs draws_args(const ecdna_ssa_ctx* c, const KeptStore& s, const ecdna_ssa_accept_draws_t& a,
                            const ecdna::accept_draws::Plan& slices, const ecdna::thin::LdsPlan& lds,
                            const void* d_cdf, const void* d_scalars) {
    const ecdna_ssa_params_t& p = c->p;
    const bool phases = &s == &c->kept_tp && c->n_passages;
    ecdna::DrawsArgs k{};
    k.headers = s.d_headers;
    k.cells = s.d_cells;
    // rule 1 as the sources 12 and 13 have it: the one summary, or on a passage context every participating phase's
    k.summaries = phases ? c->d_pas_summ : c->d_summ;
    k.err_stride = phases ? p.n_replicates : 0u;
    k.target_cdf = static_cast<const double*>(d_cdf);
    k.target_scalars = static_cast<const double*>(d_scalars);
    k.slice_mask = slices.slice_mask;
    k.rid0 = p.first_replicate;
    k.rid_stride = rid_stride(p);
    k.reps_per_set = p.reps_per_set;
    k.n = (uint32_t)p.n_replicates;
    k.m = s.m;
    k.bins = p.hist_bins;
    k.n_slices = slices.n_slices;
    k.n_targets = a.n_targets;
    k.n_sets = p.n_param_sets;
    k.first_draw = a.first_draw;
    k.n_draws = a.n_draws;
    k.reps_per_block = pass_reps_per_block(c, k.n, lds.waves);
    k.table_slots = lds.table_slots;
    k.scratch_words = lds.scratch_words;
    for (uint32_t t = 0; t < slices.n_slices; ++t) {
        const SliceStream drawn = slice_stream(c, s, t);
        k.slice_seed[t] = drawn.seed;
        k.slice_tag[t] = ecdna::thin::stream_tag(drawn.field, 0u);
    }
    return k;
}

// A threshold row as the kernels' argument blocks carry it.
void threshold_row(const ecdna_accept_threshold_t& t, double* row) {
    row[0] = t.ks;
    row[1] = t.mean_rel;
    row[2] = t.entropy_rel;
    row[3] = t.frequency_diff;
}

// ---- ecdna_ssa_ctx_select_draws / _select_draws_digits: what both do after their own argument checks ----

// The store of the block and the state checks, as draws_store makes them under select_draws::invalid.
int select_draws_store(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, KeptStore** out) {
    return draws_store(c, a, "select_draws", [&](uint32_t keep_cells) {
        return ecdna::select_draws::invalid(c->p.hist_bins, keep_cells, c->kept_tp.T, c->p.n_replicates, *a);
    }, out);
}

// The keys of every (replicate, draw) of the block, into the context's buffer, which it then holds for that block.
// n > 0. Synchronises: the uploads read host copies on this stack.
int select_draws_keys(ecdna_ssa_ctx* c, const KeptStore& s, const ecdna_ssa_accept_draws_t& a, const char* who) {
    namespace sd = ecdna::select_draws;
    const uint32_t bins = c->p.hist_bins, P = a.n_targets;
    hipStream_t st = c->last_stream;
    c->sdr_keys_valid = false;
    TRY(accept_reserve(&c->sdr_cdf, sd::cdf_bytes(P, bins), "target CDFs", who));
    TRY(accept_reserve(&c->sdr_scalars, sd::scalars_bytes(P), "target scalars", who));
    TRY(accept_reserve(&c->sdr_keys, sd::keys_bytes(c->p.n_replicates, a.n_draws), "keys", who));
    std::vector<double> host_cdf, host_scalars;
    if (const int rc = upload_targets(a.target_hists, P, bins, &host_cdf, &host_scalars, c->sdr_cdf.ptr,
                                      c->sdr_scalars.ptr, st)) {
        (void)hipStreamSynchronize(st);  // (an upload already enqueued may still read its host copy)
        return rc;
    }
    const ecdna::accept_draws::Plan pl =
        ecdna::accept_draws::plan(bins, s.m, a.timepoints == 1u, P, a.sample_cells, a.timepoint_mask);
    ecdna::SelectDrawsArgs k{};
    k.s = draws_args(c, s, a, pl, pl.lds, c->sdr_cdf.ptr, c->sdr_scalars.ptr);
    k.g = pl.grouping();
    k.keys = static_cast<uint64_t*>(c->sdr_keys.ptr);
    const hipError_t le = ecdna::launch_select_draws_keys(k, st);
    const hipError_t se = hipStreamSynchronize(st);  // (also when the launch was refused: the uploads read the stack)
    TRY(le);
    TRY(se);
    c->sdr_block = sd::remember(a, bins);
    c->sdr_keys_valid = true;
    return ECDNA_OK;
}

// One digit pass over the keys select_draws_keys made.
int select_draws_pass(ecdna_ssa_ctx* c, uint32_t n_draws, uint32_t pass, uint32_t K, const uint64_t* prefixes,
                      uint32_t stride, uint64_t* out_hist, const char* who) {
    TRY(accept_reserve(&c->sdr_hist, ecdna::select_draws::hist_bytes(), "histogram", who));
    return digit_pass(static_cast<const uint64_t*>(c->sdr_keys.ptr),
                      (uint32_t)ecdna::select_draws::n_keys(c->p.n_replicates, n_draws), c->sdr_hist.ptr, pass, K,
                      prefixes, stride, out_hist, c->last_stream);
}
}  // namespace

// library-internal entry points for ssa_comm.cpp (the RCCL reduction)
__attribute__((visibility("hidden"))) int ecdna_ssa_internal_fail(int code, const std::string& msg) {
    return fail(code, msg);
}

__attribute__((visibility("hidden"))) int ecdna_ssa_internal_ctx_outputs(ecdna_ssa_ctx* c, uint64_t** d_hist,
                                                                         ecdna_totals_t** d_tot, uint32_t* n_sets,
                                                                         uint32_t* bins, int* device, void** stream) {
    TRY(ctx_launched(c, "reduce before launch"));
    *d_hist = c->d_hist;
    *d_tot = c->d_tot;
    *n_sets = c->p.n_param_sets;
    *bins = c->p.hist_bins;
    *device = c->device;
    *stream = c->last_stream;
    return ECDNA_OK;
}

extern "C" {

int ecdna_ssa_abi_version(void) { return ECDNA_SSA_ABI_VERSION; }

// (development / test entry point, not part of include/ecdna_ssa.h: bin_schedule_rule for the CPU tests)
int ecdna_dev_bin_schedule(int pair_ok, uint64_t pair_mode, uint64_t sched, uint64_t max_chunk, uint32_t cus,
                           int k64u16, int tf0, int occ_def, int occ_ilp, uint32_t stepper_block) {
    return ecdna::plan::bin_schedule_rule(pair_ok != 0, pair_mode, sched, max_chunk, cus, k64u16 != 0, tf0 != 0, occ_def,
                                          occ_ilp, stepper_block);
}

// (development / test entry point, not part of include/ecdna_ssa.h: the sampling passes' LDS plan of ssa_launch.h for
// the CPU tests. pass 0 = ssa_subsample, 1 = ssa_passage, 2 = ssa_snapstats, where m = 0 means no samples; the passes
// of the keep block: 3 = the keep pass, 4 = ssa_rescore, 5 = ssa_pool_accepted, the last two whatever m and bag_k; of the
// timepoint keep block: 6 = the snapshot keep pass, whatever bag_k — its populations are rows)
int ecdna_dev_pass_lds(int pass, uint32_t bins, uint32_t bag_k, uint32_t m, uint32_t* waves, uint64_t* lds_bytes,
                       int* sample_hist_lds) {
    if (pass < 0 || pass > 6 || (!m && pass != 2 && pass != 4 && pass != 5) || !waves || !lds_bytes || !sample_hist_lds)
        return fail(ECDNA_E_INVALID, "ecdna_dev_pass_lds: unknown pass, m = 0 outside pass 2, or a NULL output");
    const uint32_t slots = m ? ecdna::subsample_table_slots(m) : 0u;
    size_t lds = 0;
    bool in_lds = false;
    *waves = pass == 0   ? ecdna::subsample_waves(bins, bag_k, slots, &lds)
             : pass == 1 ? ecdna::passage_waves(bins, bag_k, slots, ecdna::passage_sort_slots(m), &lds)
             : pass == 3 ? ecdna::keep_waves(bins, bag_k, slots, ecdna::passage_sort_slots(m), &lds)
             : pass == 4 ? ecdna::rescore_waves(bins, &lds)
             : pass == 5 ? ecdna::pool_accepted_waves(bins, &lds)
             : pass == 6 ? ecdna::keep_snapshots_waves(bins, slots, ecdna::passage_sort_slots(m), &lds)
                         : ecdna::snapstats_waves(bins, slots, &lds, &in_lds);
    *lds_bytes = lds;
    *sample_hist_lds = in_lds ? 1 : 0;
    return ECDNA_OK;
}

const char* ecdna_ssa_strerror(int code) {
    switch (code) {
        case ECDNA_OK: return "ok";
        case ECDNA_E_INVALID: return "invalid argument";
        case ECDNA_E_HIP: return "HIP runtime error";
        case ECDNA_E_NOMEM: return "device out of memory";
        case ECDNA_E_NODEVICE: return "no usable gfx950 device";
        case ECDNA_E_STATE: return "invalid call order";
        case ECDNA_E_COMM: return "RCCL communication error (or librccl.so.1 missing)";
        default: return "unknown error";
    }
}

const char* ecdna_ssa_last_error_message(void) { return g_last_error.c_str(); }

int ecdna_ssa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int good = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            ++good;
    }
    return good;
}

int ecdna_ssa_ctx_create(const ecdna_ssa_params_t* p, ecdna_ssa_ctx** out) {
    return ecdna_ssa_ctx_create_ext(p, nullptr, out);
}

int ecdna_ssa_ctx_create_ext(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext, ecdna_ssa_ctx** out) {
    return ecdna_ssa_ctx_create_passages(p, ext, nullptr, out);
}

int ecdna_ssa_ctx_create_passages(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                  const ecdna_ssa_passages_t* pas, ecdna_ssa_ctx** out) {
    return ecdna_ssa_ctx_create_cohort(p, ext, pas, nullptr, out);
}

int ecdna_ssa_ctx_create_cohort(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                const ecdna_ssa_passages_t* pas, const ecdna_ssa_cohort_t* co, ecdna_ssa_ctx** out) {
    return ecdna_ssa_ctx_create_keep(p, ext, pas, co, nullptr, out);
}

int ecdna_ssa_ctx_create_keep(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext, const ecdna_ssa_passages_t* pas,
                              const ecdna_ssa_cohort_t* co, const ecdna_ssa_keep_t* keep, ecdna_ssa_ctx** out) {
    return ecdna_ssa_ctx_create_keep_timepoints(p, ext, pas, co, keep, nullptr, out);
}

int ecdna_ssa_ctx_create_keep_timepoints(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                         const ecdna_ssa_passages_t* pas, const ecdna_ssa_cohort_t* co,
                                         const ecdna_ssa_keep_t* keep, const ecdna_ssa_keep_timepoints_t* kt,
                                         ecdna_ssa_ctx** out) {
    if (!out) return fail(ECDNA_E_INVALID, "out is NULL");
    *out = nullptr;
    TRY(validate(p, ext, pas));
    if (co) {  // the cohort block
        const std::string why = ecdna::cohort::invalid(*p, ext, pas, *co);
        if (!why.empty()) return fail(ECDNA_E_INVALID, why);
    }
    if (keep) {  // the keep block
        const std::string why = ecdna::keep::invalid(*p, pas, *keep);
        if (!why.empty()) return fail(ECDNA_E_INVALID, why);
    }
    if (kt) {  // the timepoint keep block
        const std::string why = ecdna::keep_timepoints::invalid(*p, ext, pas, *kt);
        if (!why.empty()) return fail(ECDNA_E_INVALID, why);
    }
    TRY(pick_device(p->device));
    ecdna_ssa_ctx* c = new ecdna_ssa_ctx();
    if (int rc = build_ctx(c, p, ext, pas, co, keep, kt)) {
        free_ctx(c);
        return rc;
    }
    *out = c;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_set_outputs(ecdna_ssa_ctx* c, uint64_t* d_hist, ecdna_totals_t* d_totals) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    c->d_hist = d_hist ? d_hist : c->d_hist_own;
    c->d_tot = d_totals ? d_totals : c->d_tot_own;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_launch(ecdna_ssa_ctx* c, void* stream) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the default (null) stream
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t nb = (uint64_t)p.n_param_sets * p.hist_bins;
    TRY(hipMemsetAsync(c->d_hist, 0, nb * sizeof(uint64_t), st));
    TRY(hipMemsetAsync(c->d_tot, 0, p.n_param_sets * sizeof(ecdna_totals_t), st));
    if (c->d_sample_hist) TRY(hipMemsetAsync(c->d_sample_hist, 0, nb * sizeof(uint64_t), st));
    if (c->d_snap_hist) TRY(hipMemsetAsync(c->d_snap_hist, 0, p.n_snapshots * nb * sizeof(uint64_t), st));
    if (c->d_snap_sample_hist)
        TRY(hipMemsetAsync(c->d_snap_sample_hist, 0, p.n_snapshots * nb * sizeof(uint64_t), st));
    if (!c->chunks.empty())
        TRY(hipMemsetAsync(c->d_heads, 0, c->chunks.size() * sizeof(uint32_t), st));
    if (c->d_snap_meta)
        TRY(hipMemsetAsync(c->d_snap_meta, 0, p.n_replicates * p.n_snapshots * sizeof(ecdna_snapshot_t), st));
    // a passage run: G growth phases per chunk, phase g into its own slice of the per-phase outputs
    const uint32_t G = std::max<uint32_t>(c->n_passages, 1u);
    const uint64_t n_run = std::max<uint64_t>(p.n_replicates, 1);
    if (c->n_passages) {
        TRY(hipMemsetAsync(c->d_pas_hist, 0, G * nb * sizeof(uint64_t), st));
        TRY(hipMemsetAsync(c->d_pas_sample_hist, 0, G * nb * sizeof(uint64_t), st));
        TRY(hipMemsetAsync(c->d_pas_tot, 0, (uint64_t)G * p.n_param_sets * sizeof(ecdna_totals_t), st));
    }

    for (size_t k = 0; k < c->chunks.size(); ++k)
        for (uint32_t g = 0; g < G; ++g) TRY(launch_chunk_phase(c, k, g, st));
    if (c->n_passages && p.n_replicates) {  // the ordinary outputs are the last phase's
        const uint64_t at = (G - 1u) * n_run;
        TRY(copy_async(c->d_summ, c->d_pas_summ + at, p.n_replicates, st));
        TRY(copy_async(c->d_stats, c->d_pas_stats + at, p.n_replicates, st));
        TRY(copy_async(c->d_sample_stats, c->d_pas_sample_stats + at, p.n_replicates, st));
    }
    if (c->n_passages) {
        const uint64_t gl = G - 1u;
        TRY(copy_async(c->d_hist, c->d_pas_hist + gl * nb, nb, st));
        TRY(copy_async(c->d_sample_hist, c->d_pas_sample_hist + gl * nb, nb, st));
        TRY(copy_async(c->d_tot, c->d_pas_tot + gl * p.n_param_sets, p.n_param_sets, st));
    }
    c->last_stream = st;
    c->launched = true;
    c->accept_valid = false;  // (the acceptance pass's results were the previous launch's)
    c->sel_keys_valid = false;  // (and the select passes' keys were made from its records)
    c->kept.valid = c->kept_tp.valid = false;  // (and the rescored records from its kept samples)
    c->adr_valid = false;  // (and the thinned acceptance's counts)
    c->sdr_keys_valid = false;  // (and the select over thinning draws' keys)
    return ECDNA_OK;
}

int ecdna_ssa_ctx_sync(ecdna_ssa_ctx* c, float* ssa_ms, float* hist_ms) {
    TRY(ctx_launched(c, "sync before launch"));
    TRY(ctx_drain(c));
    float s = 0.f, h = 0.f;
    for (auto& ch : c->chunks) {
        for (size_t e = 0; e + 2 < ch.ev.size(); e += 3) {  // per growth phase (one in an ordinary run)
            float a = 0.f, b = 0.f;
            TRY(hipEventElapsedTime(&a, ch.ev[e], ch.ev[e + 1]));
            TRY(hipEventElapsedTime(&b, ch.ev[e + 1], ch.ev[e + 2]));
            s += a;
            h += b;
        }
    }
    if (ssa_ms) *ssa_ms = s;
    if (hist_ms) *hist_ms = h;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_device_outputs(ecdna_ssa_ctx* c, uint64_t** d_hist, ecdna_totals_t** d_totals) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (d_hist) *d_hist = c->d_hist;
    if (d_totals) *d_totals = c->d_tot;
    return ECDNA_OK;
}

int64_t ecdna_ssa_ctx_row_stride(const ecdna_ssa_ctx* c) {
    if (!c) return 0;
    return c->chunks.size() <= 1 ? (int64_t)c->out_stride : 0;
}

int ecdna_ssa_ctx_geometry(const ecdna_ssa_ctx* c, uint64_t* chunk_replicates, uint64_t* grid_lanes) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (chunk_replicates) *chunk_replicates = c->chunk_reps;
    if (grid_lanes) *grid_lanes = (uint64_t)c->stepper_blocks_cap * c->stepper_block;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_instance(const ecdna_ssa_ctx* c, ecdna_ssa_instance_t* out) {
    if (!c || !out) return fail(ECDNA_E_INVALID, "ctx / out is NULL");
    ecdna_ssa_instance_t r{};
    const void* fn = stepper_fn(*c, c->window, c->bin_ilp);
    if (c->refdraws) {
        r.kernel = ECDNA_KERNEL_REFDRAWS;
        r.schedule = -1;
    } else if (c->bin_k) {
        r.kernel = ECDNA_KERNEL_BINS;
        r.schedule = c->bin_ilp;
        r.paired = c->bin_ilp == 3 ? 1 : 0;
        r.bin_kmax = c->bin_k;
        r.bin_c32 = (uint32_t)c->bin_c32;
        r.runtime_flags = (kernel_flags(*c) & ecdna::kRuntimeFlagMask) ? 1 : 0;
    } else {
        r.kernel = ECDNA_KERNEL_ROWS;
        r.schedule = -1;
        r.window = (uint32_t)c->window;
        r.runtime_flags = 1;
    }
    for (const auto& ch : c->chunks) {
        r.rotation += ch.rot_n_pad ? 1 : 0;
        r.drain_control += ch.admit_slot != 0xffffffffu ? 1 : 0;
    }
    r.rot_tick_log2 = (int32_t)c->rot_tick_log2;
    r.cost_order = c->d_order ? 1 : 0;
    r.block_lanes = c->stepper_block;
    r.cus = (uint32_t)c->cus;
    // the grid actually launched (the largest chunk's; a small or paired run launches fewer blocks than the
    // occupancy cap), and its workgroups per CU rounded up
    uint32_t launched = 0;
    for (const auto& ch : c->chunks) launched = std::max<uint32_t>(launched, ch.blocks);
    r.blocks_per_cu = c->cus ? (launched + (uint32_t)c->cus - 1u) / (uint32_t)c->cus : 0u;
    r.n_chunks = (uint32_t)c->chunks.size();
    r.chunk_replicates = c->chunk_reps;
    r.grid_lanes = (uint64_t)launched * c->stepper_block;
    hipFuncAttributes fa{};
    if (fn && hipFuncGetAttributes(&fa, fn) == hipSuccess) {
        r.vgprs = (uint32_t)fa.numRegs;
        r.lds_bytes = (uint32_t)fa.sharedSizeBytes;
        r.scratch_bytes = (uint32_t)fa.localSizeBytes;
    }
    *out = r;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download(ecdna_ssa_ctx* c, ecdna_rep_summary_t* out_summaries, uint64_t* out_hist,
                           ecdna_totals_t* out_totals, uint16_t* out_rows) {
    TRY(ctx_launched(c));
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n = p.n_replicates;
    if (out_summaries && n) TRY(to_host(out_summaries, c->d_summ, n));
    if (out_hist) TRY(to_host(out_hist, c->d_hist, (uint64_t)p.n_param_sets * p.hist_bins));
    if (out_totals) TRY(to_host(out_totals, c->d_tot, p.n_param_sets));
    if (out_rows) {
        if (c->chunks.size() > 1) return fail(ECDNA_E_STATE, "rows are not downloadable from a chunked run");
        if (n && !c->bin_k) TRY(to_host(out_rows, c->d_rows, n * c->row_stride));
        if (c->bin_k && n) {
            std::vector<uint16_t> dev_rows(n * c->row_stride);  // the large-k rows
            TRY(to_host(dev_rows.data(), c->d_rows, dev_rows.size()));
            // bin store: canonical rows = the counters expanded (k ascending), then the large-k row
            std::vector<ecdna_rep_summary_t> summ(n);
            TRY(to_host(summ.data(), c->d_summ, n));
            const uint64_t kb = c->bin_k;
            std::vector<uint32_t> bags(n * kb);
            if (c->bin_c32) {
                TRY(to_host(bags.data(), reinterpret_cast<const uint32_t*>(c->d_bags), bags.size()));
            } else {
                std::vector<uint16_t> b16(bags.size());
                TRY(to_host(b16.data(), reinterpret_cast<const uint16_t*>(c->d_bags), b16.size()));
                std::copy(b16.begin(), b16.end(), bags.begin());
            }
            std::vector<uint16_t> big;
            for (uint64_t i = 0; i < n; ++i) {
                uint16_t* r = out_rows + i * c->out_stride;
                const uint16_t* dr = dev_rows.data() + i * c->row_stride;
                uint64_t small = 0;
                for (uint64_t b = 0; b < kb; ++b) small += bags[i * kb + b];
                const uint64_t nbig = std::min<uint64_t>(summ[i].nplus >= small ? summ[i].nplus - small : 0,
                                                         c->row_stride);
                big.assign(dr, dr + nbig);
                uint64_t pos = 0;
                for (uint64_t b = 0; b < kb; ++b)
                    for (uint32_t q = 0; q < bags[i * kb + b] && pos < c->out_stride; ++q) r[pos++] = (uint16_t)(b + 1);
                const uint64_t tail = std::min<uint64_t>(big.size(), c->out_stride - pos);
                std::copy(big.begin(), big.begin() + tail, r + pos);
            }
        }
    }
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_snapshots(ecdna_ssa_ctx* c, ecdna_snapshot_t* meta, uint16_t* rows) {
    TRY(ctx_launched(c));
    const ecdna_ssa_params_t& p = c->p;
    if (!p.n_snapshots || !p.n_replicates) return ECDNA_OK;
    TRY(ctx_drain(c));
    const uint64_t ns = p.n_replicates * p.n_snapshots;
    if (meta) TRY(to_host(meta, c->d_snap_meta, ns));
    if (rows) {
        if (!c->d_snap_rows || c->snap_rows_local)
            return fail(ECDNA_E_STATE, "snapshot rows need ECDNA_FLAG_SNAPSHOT_ROWS");
        TRY(to_host(rows, c->d_snap_rows, ns * c->out_stride));
    }
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_stats(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out) {
    TRY(ctx_launched(c));
    if (!c->d_stats) return fail(ECDNA_E_STATE, "statistics need ECDNA_FLAG_REP_STATS");
    if (!out || !c->p.n_replicates) return ECDNA_OK;
    TRY(ctx_drain(c));
    TRY(to_host(out, c->d_stats, c->p.n_replicates));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_sample(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats, uint64_t* out_sample_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->d_sample_hist) return fail(ECDNA_E_STATE, "the sample needs subsample_cells > 0");
    TRY(ctx_launched(c));
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    if (out_stats && p.n_replicates) TRY(to_host(out_stats, c->d_sample_stats, p.n_replicates));
    if (out_sample_hist) TRY(to_host(out_sample_hist, c->d_sample_hist, (uint64_t)p.n_param_sets * p.hist_bins));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_snapshot_stats(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats,
                                          ecdna_rep_stats_t* out_sample_stats, uint64_t* out_hist,
                                          uint64_t* out_sample_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->snap_stats) return fail(ECDNA_E_STATE, "snapshot statistics need ecdna_ssa_ext_t.snapshot_stats");
    TRY(ctx_launched(c));
    if ((out_sample_stats || out_sample_hist) && !c->snap_m)
        return fail(ECDNA_E_STATE, "the snapshot samples need ecdna_ssa_ext_t.snapshot_subsample_cells > 0");
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t ns = p.n_replicates * p.n_snapshots;
    const uint64_t hb = (uint64_t)p.n_snapshots * p.n_param_sets * p.hist_bins;
    if (out_stats && ns) TRY(to_host(out_stats, c->d_snap_stats, ns));
    if (out_sample_stats && ns) TRY(to_host(out_sample_stats, c->d_snap_sample_stats, ns));
    if (out_hist) TRY(to_host(out_hist, c->d_snap_hist, hb));
    if (out_sample_hist) TRY(to_host(out_sample_hist, c->d_snap_sample_hist, hb));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_passages(ecdna_ssa_ctx* c, ecdna_rep_summary_t* out_summaries, ecdna_totals_t* out_totals,
                                    ecdna_rep_stats_t* out_stats, ecdna_rep_stats_t* out_sample_stats,
                                    uint64_t* out_hist, uint64_t* out_sample_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->n_passages) return fail(ECDNA_E_STATE, "per-phase results need ecdna_ssa_ctx_create_passages");
    TRY(ctx_launched(c));
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t G = c->n_passages, n = p.n_replicates;
    const uint64_t hb = G * p.n_param_sets * p.hist_bins;
    if (out_summaries && n) TRY(to_host(out_summaries, c->d_pas_summ, G * n));
    if (out_totals) TRY(to_host(out_totals, c->d_pas_tot, G * p.n_param_sets));
    if (out_stats && n) TRY(to_host(out_stats, c->d_pas_stats, G * n));
    if (out_sample_stats && n) TRY(to_host(out_sample_stats, c->d_pas_sample_stats, G * n));
    if (out_hist) TRY(to_host(out_hist, c->d_pas_hist, hb));
    if (out_sample_hist) TRY(to_host(out_sample_hist, c->d_pas_sample_hist, hb));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_cohort(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats, ecdna_rep_stats_t* out_sample_stats) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->n_cohort) return fail(ECDNA_E_STATE, "the cohort records need ecdna_ssa_ctx_create_cohort");
    TRY(ctx_launched(c));
    if (out_sample_stats && !c->d_coh_sample_stats)
        return fail(ECDNA_E_STATE, "the cohort samples need ecdna_ssa_cohort_t.sample_cells");
    TRY(ctx_drain(c));
    const uint64_t records = (uint64_t)c->n_cohort * c->p.n_replicates;
    if (out_stats && records) TRY(to_host(out_stats, c->d_coh_stats, records));
    if (out_sample_stats && records) TRY(to_host(out_sample_stats, c->d_coh_sample_stats, records));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_accept(ecdna_ssa_ctx* c, const ecdna_ssa_accept_t* a) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!a) return fail(ECDNA_E_INVALID, "accept is NULL");
    if (a->struct_size != sizeof(ecdna_ssa_accept_t))
        return fail(ECDNA_E_INVALID, "accept.struct_size must be sizeof(ecdna_ssa_accept_t)");
    if (!is_accept_source(a->source))
        return fail(ECDNA_E_INVALID, "accept.source is not an ecdna_accept_source_t");
    if (a->n_thresholds < 1u || a->n_thresholds > ecdna::kMaxAcceptRows)
        return fail(ECDNA_E_INVALID, "accept.n_thresholds must be in [1, 32]");
    if (a->list_threshold >= a->n_thresholds)
        return fail(ECDNA_E_INVALID, "accept.list_threshold must be < n_thresholds");
    if (!a->thresholds) return fail(ECDNA_E_INVALID, "accept.thresholds is NULL");
    for (uint32_t q = 0; q < a->n_thresholds; ++q) {
        const ecdna_accept_threshold_t& t = a->thresholds[q];
        const double v[4] = {t.ks, t.mean_rel, t.entropy_rel, t.frequency_diff};
        const char* names[4] = {"ks", "mean_rel", "entropy_rel", "frequency_diff"};
        for (int k = 0; k < 4; ++k)
            if (!(v[k] >= 0.0))
                return fail(ECDNA_E_INVALID, "accept.thresholds[" + std::to_string(q) + "]." + names[k] +
                                                 " must be >= 0 (+inf switches it off) and not NaN");
    }
    if (a->reserved) return fail(ECDNA_E_INVALID, "accept.reserved must be 0");
    const ecdna_ssa_params_t& p = c->p;
    if (p.n_replicates >= (1ull << 32)) return fail(ECDNA_E_INVALID, "accept: n_replicates must be < 2^32");
    AcceptSource src;
    TRY(accept_source(c, a->source, &src));
    const uint64_t all = src.T >= 64u ? ~0ull : (1ull << src.T) - 1ull;
    if (a->timepoint_mask & ~all)
        return fail(ECDNA_E_INVALID, "accept.timepoint_mask has bits at or above T = " + std::to_string(src.T));
    TRY(ctx_launched(c, "accept before launch"));
    if (!src.has_target)
        return fail(ECDNA_E_STATE, "accept: the source's statistics were computed without a target (every distance is "
                                   "0: nothing could be rejected)");

    const uint64_t n = p.n_replicates;
    const uint32_t Q = a->n_thresholds;
    const uint64_t list_cap = std::min<uint64_t>(a->list_capacity, n);
    const uint32_t n_blocks = (uint32_t)((n + ecdna::kAcceptBlock - 1) / ecdna::kAcceptBlock);
    c->accept_valid = false;
    TRY(hipSetDevice(c->device));
    TRY(accept_reserve(&c->acc_counts, (uint64_t)Q * p.n_param_sets * sizeof(uint64_t), "counts"));
    if (n) TRY(accept_reserve(&c->acc_mask, n * sizeof(uint32_t), "mask"));
    if (list_cap) {
        TRY(accept_reserve(&c->acc_blocks, (uint64_t)n_blocks * sizeof(uint32_t), "workgroup counts"));
        TRY(accept_reserve(&c->acc_ids, list_cap * sizeof(uint64_t), "list ids"));
        TRY(accept_reserve(&c->acc_list, list_cap * src.T * sizeof(ecdna_rep_stats_t), "list records"));
    }

    hipStream_t st = c->last_stream;
    TRY(hipMemsetAsync(c->acc_counts.ptr, 0, (uint64_t)Q * p.n_param_sets * sizeof(uint64_t), st));
    if (n) {
        ecdna::AcceptArgs k{};
        k.stats = src.stats;
        k.summaries = src.summaries;
        k.rep_stride = src.rep_stride;
        k.tp_stride = src.tp_stride;
        k.err_stride = src.err_stride;
        k.tmask = a->timepoint_mask ? a->timepoint_mask : all;
        k.rid0 = p.first_replicate;
        k.rid_stride = rid_stride(p);
        k.reps_per_set = p.reps_per_set;
        k.n = (uint32_t)n;
        k.T = src.T;
        k.Q = Q;
        k.n_sets = p.n_param_sets;
        k.mask = static_cast<uint32_t*>(c->acc_mask.ptr);
        k.counts = static_cast<unsigned long long*>(c->acc_counts.ptr);
        k.list_q = a->list_threshold;
        k.n_blocks = n_blocks;
        k.block_counts = static_cast<uint32_t*>(c->acc_blocks.ptr);
        k.list_capacity = list_cap;
        k.ids = static_cast<uint64_t*>(c->acc_ids.ptr);
        k.list_stats = static_cast<ecdna_rep_stats_t*>(c->acc_list.ptr);
        for (uint32_t q = 0; q < Q; ++q) {
            const ecdna_accept_threshold_t& t = a->thresholds[q];
            k.thr[q][0] = t.ks;
            k.thr[q][1] = t.mean_rel;
            k.thr[q][2] = t.entropy_rel;
            k.thr[q][3] = t.frequency_diff;
        }
        TRY(ecdna::launch_accept_mask(k, st));
        if (list_cap) TRY(ecdna::launch_accept_list(k, st));
    }
    c->acc_rows = Q;
    c->acc_timepoints = src.T;
    c->acc_list_row = a->list_threshold;
    c->acc_list_cap = list_cap;
    c->accept_valid = true;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_accept(ecdna_ssa_ctx* c, uint64_t* out_counts, uint32_t* out_mask,
                                  uint64_t* out_n_accepted, uint64_t* out_ids,
                                  ecdna_rep_stats_t* out_list_stats) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched || !c->accept_valid)
        return fail(ECDNA_E_STATE, "download_accept before accept (a launch invalidates the acceptance results)");
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t* d_counts = static_cast<const uint64_t*>(c->acc_counts.ptr);
    // the number accepted under the list's row: the sum of its counts over the sets
    std::vector<uint64_t> row(p.n_param_sets);
    TRY(to_host(row.data(), d_counts + (uint64_t)c->acc_list_row * p.n_param_sets, p.n_param_sets));
    uint64_t n_accepted = 0;
    for (const uint64_t x : row) n_accepted += x;
    if (out_n_accepted) *out_n_accepted = n_accepted;
    if (out_counts) TRY(to_host(out_counts, d_counts, (uint64_t)c->acc_rows * p.n_param_sets));
    if (out_mask && p.n_replicates)
        TRY(to_host(out_mask, static_cast<const uint32_t*>(c->acc_mask.ptr), p.n_replicates));
    const uint64_t listed = std::min<uint64_t>(n_accepted, c->acc_list_cap);
    if (out_ids && listed) TRY(to_host(out_ids, static_cast<const uint64_t*>(c->acc_ids.ptr), listed));
    if (out_list_stats && listed)
        TRY(to_host(out_list_stats, static_cast<const ecdna_rep_stats_t*>(c->acc_list.ptr),
                    listed * c->acc_timepoints));
    return ECDNA_OK;
}

// ---- the calls over the kept samples, of the keep block (ecdna_ssa_keep_t) and of the timepoint keep block
// (ecdna_ssa_keep_timepoints_t): each checks its own arguments, in its own order and words, and runs the pass over its
// block's store ----

int ecdna_ssa_ctx_rescore(ecdna_ssa_ctx* c, uint32_t n_targets, const uint64_t* target_hists) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (n_targets < 1u || n_targets > ecdna::kMaxCohortTargets)
        return fail(ECDNA_E_INVALID, "rescore.n_targets must be in [1, 64]");
    if (!target_hists) return fail(ECDNA_E_INVALID, "rescore.target_hists is NULL");
    const uint32_t empty = first_empty_target(target_hists, n_targets, c->p.hist_bins);
    if (empty < n_targets)
        return fail(ECDNA_E_INVALID, "rescore.target_hists[" + std::to_string(empty) + "] is empty");
    if (!c->kept.m) return fail(ECDNA_E_STATE, "rescore: the kept samples need ecdna_ssa_ctx_create_keep");
    TRY(ctx_launched(c, "rescore before launch"));
    return rescore_store(c, &c->kept, n_targets, target_hists, "ecdna_ssa_ctx_rescore");
}

int ecdna_ssa_ctx_rescore_timepoints(ecdna_ssa_ctx* c, const uint64_t* target_hists) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!target_hists) return fail(ECDNA_E_INVALID, "rescore_timepoints.target_hists is NULL");
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("rescore_timepoints") + kNeedsTimepoints);
    const uint32_t T = c->kept_tp.T, empty = first_empty_target(target_hists, T, c->p.hist_bins);
    if (empty < T)
        return fail(ECDNA_E_INVALID, "rescore_timepoints.target_hists[" + std::to_string(empty) + "] is empty");
    TRY(ctx_launched(c, "rescore_timepoints before launch"));
    // timepoint t's samples against target t: one target per slice
    return rescore_store(c, &c->kept_tp, 1u, target_hists, "ecdna_ssa_ctx_rescore_timepoints");
}

int ecdna_ssa_ctx_rescore_sized(ecdna_ssa_ctx* c, const ecdna_ssa_rescore_t* r) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!r) return fail(ECDNA_E_INVALID, "rescore_sized: the block is NULL");
    const std::string bad = ecdna::thin::invalid(c->p.hist_bins, c->kept.m ? c->kept.m : ecdna::kMaxSubsampleCells, *r);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    if (!c->kept.m) return fail(ECDNA_E_STATE, "rescore_sized: the kept samples need ecdna_ssa_ctx_create_keep");
    TRY(ctx_launched(c, "rescore_sized before launch"));
    // (no sizes: every target on the whole kept sample, the unsized call's pass; the draws then thin nothing)
    const ThinSizes sizes{r->sample_cells, r->sample_draws};
    return rescore_store(c, &c->kept, r->n_targets, r->target_hists, "ecdna_ssa_ctx_rescore_sized",
                         r->sample_cells ? &sizes : nullptr);
}

int ecdna_ssa_ctx_rescore_timepoints_sized(ecdna_ssa_ctx* c, const uint64_t* target_hists, const uint32_t* sample_cells,
                                           uint32_t draw) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!target_hists) return fail(ECDNA_E_INVALID, "rescore_timepoints_sized.target_hists is NULL");
    if (draw > ecdna::thin::kMaxDraw) return fail(ECDNA_E_INVALID, "rescore_timepoints_sized.draw must be in [0, 63]");
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("rescore_timepoints_sized") + kNeedsTimepoints);
    const uint32_t T = c->kept_tp.T;
    const std::string bad =
        ecdna::thin::invalid_timepoints(c->p.hist_bins, c->kept_tp.m, T, target_hists, sample_cells, draw);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    TRY(ctx_launched(c, "rescore_timepoints_sized before launch"));
    // timepoint t's samples against target t on sample_cells[t] cells: one target per slice, all on draw `draw`
    const std::vector<uint32_t> draws(T, draw);
    const ThinSizes sizes{sample_cells, draws.data()};
    return rescore_store(c, &c->kept_tp, 1u, target_hists, "ecdna_ssa_ctx_rescore_timepoints_sized",
                         sample_cells ? &sizes : nullptr);
}

// ---- the acceptance over repeated thinnings of the kept samples (thinned acceptance mapping v1): ssa_thin and the
// acceptance pass run together over a range of draws, on buffers of its own ----

int ecdna_ssa_ctx_accept_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a) {
    namespace ad = ecdna::accept_draws;
    const char* who = "ecdna_ssa_ctx_accept_draws";
    KeptStore* s = nullptr;
    TRY(draws_store(c, a, "accept_draws", [&](uint32_t keep_cells) {
        return ad::invalid(c->p.hist_bins, keep_cells, c->kept_tp.T, c->p.n_replicates, *a);
    }, &s));

    const ecdna_ssa_params_t& p = c->p;
    const uint32_t bins = p.hist_bins, Q = a->n_thresholds, P = a->n_targets;
    const uint64_t n = p.n_replicates;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    // an earlier call may still read the targets this one replaces (and its upload their host copies)
    if (c->adr_pending) TRY(hipStreamSynchronize(c->adr_stream));
    c->adr_pending = false;
    c->adr_valid = false;
    TRY(accept_reserve(&c->adr_cdf, ad::cdf_bytes(P, bins), "target CDFs", who));
    TRY(accept_reserve(&c->adr_scalars, ad::scalars_bytes(P), "target scalars", who));
    TRY(accept_reserve(&c->adr_sums, ad::sums_bytes(Q, p.n_param_sets), "sums", who));
    if (n) TRY(accept_reserve(&c->adr_passes, ad::passes_bytes(n, Q), "passes", who));
    TRY(hipMemsetAsync(c->adr_sums.ptr, 0, ad::sums_bytes(Q, p.n_param_sets), st));
    if (n) {
        // (the call only enqueues: the uploads' host copies live in the context)
        TRY(upload_targets(a->target_hists, P, bins, &c->adr_host_cdf, &c->adr_host_scalars, c->adr_cdf.ptr,
                           c->adr_scalars.ptr, st));
        c->adr_pending = true;
        c->adr_stream = st;
        const ad::Plan pl = ad::plan(bins, s->m, a->timepoints == 1u, P, a->sample_cells, a->timepoint_mask);
        ecdna::AcceptDrawsArgs k{};
        k.s = draws_args(c, *s, *a, pl, pl.lds, c->adr_cdf.ptr, c->adr_scalars.ptr);
        k.g = pl.grouping();
        k.passes = static_cast<uint8_t*>(c->adr_passes.ptr);
        k.sums = static_cast<unsigned long long*>(c->adr_sums.ptr);
        k.Q = Q;
        for (uint32_t q = 0; q < Q; ++q) threshold_row(a->thresholds[q], k.thr[q]);
        TRY(ecdna::launch_accept_draws(k, st));
    }
    c->adr_rows = Q;
    c->adr_valid = true;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_accept_draws(ecdna_ssa_ctx* c, uint64_t* out_sums, uint8_t* out_passes) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched || !c->adr_valid)
        return fail(ECDNA_E_STATE, "download_accept_draws before accept_draws (a launch invalidates its results)");
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    if (out_sums)
        TRY(to_host(out_sums, static_cast<const uint64_t*>(c->adr_sums.ptr), (uint64_t)c->adr_rows * p.n_param_sets));
    if (out_passes && p.n_replicates)
        TRY(to_host(out_passes, static_cast<const uint8_t*>(c->adr_passes.ptr), p.n_replicates * c->adr_rows));
    return ECDNA_OK;
}

// ---- the accepted thinnings pooled (thinned pooling mapping v1): the verdict of ecdna_ssa_ctx_accept_draws for one
// row and the pools of what passes it, in one synchronous pass on buffers of its own ----

int ecdna_ssa_ctx_pool_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t threshold,
                             uint64_t* out_thinned, uint64_t* out_kept) {
    namespace pd = ecdna::pool_draws;
    const char* who = "ecdna_ssa_ctx_pool_draws";
    KeptStore* s = nullptr;
    TRY(draws_store(c, a, "pool_draws", [&](uint32_t keep_cells) {
        return pd::invalid(c->p.hist_bins, keep_cells, c->kept_tp.T, c->p.n_replicates, *a, threshold, out_thinned,
                           out_kept);
    }, &s));

    const ecdna_ssa_params_t& p = c->p;
    const uint32_t bins = p.hist_bins, P = a->n_targets, sets = p.n_param_sets;
    const uint64_t n = p.n_replicates;
    const pd::Plan pl = pd::plan(bins, s->m, a->timepoints == 1u, P, a->sample_cells, a->timepoint_mask);
    const uint32_t S = pl.pool.n_slices;
    const uint64_t thinned_words = pd::thinned_words(P, sets, bins), kept_words = pd::kept_words(S, sets, bins);
    if (out_thinned) std::fill(out_thinned, out_thinned + thinned_words, 0ull);
    if (out_kept) std::fill(out_kept, out_kept + kept_words, 0ull);
    if (!n) return ECDNA_OK;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    TRY(accept_reserve(&c->pdr_cdf, pd::cdf_bytes(P, bins), "target CDFs", who));
    TRY(accept_reserve(&c->pdr_scalars, pd::scalars_bytes(P), "target scalars", who));
    TRY(accept_reserve(&c->pdr_pool, pd::pooled_bytes(P, S, sets, bins), "pooled histograms", who));
    unsigned long long* d_thinned = static_cast<unsigned long long*>(c->pdr_pool.ptr);
    unsigned long long* d_kept = d_thinned + thinned_words;
    TRY(hipMemsetAsync(c->pdr_pool.ptr, 0, pd::pooled_bytes(P, S, sets, bins), st));
    // (the call synchronises below, so the uploads' host copies live on its stack)
    std::vector<double> host_cdf, host_scalars;
    if (const int rc = upload_targets(a->target_hists, P, bins, &host_cdf, &host_scalars, c->pdr_cdf.ptr,
                                      c->pdr_scalars.ptr, st)) {
        (void)hipStreamSynchronize(st);  // (an upload already enqueued may still read its host copy)
        return rc;
    }

    ecdna::PoolDrawsArgs k{};
    // (the slices and the mask are the verdict's: the pooling grouping walks every slice whatever the mask)
    k.s = draws_args(c, *s, *a, pl.verdict, pl.lds, c->pdr_cdf.ptr, c->pdr_scalars.ptr);
    k.verdict = pl.verdict.grouping();
    k.pool = pl.pool.grouping();
    k.thinned = out_thinned ? d_thinned : nullptr;
    k.kept = out_kept ? d_kept : nullptr;
    k.wave_words = ecdna::pool_draws_wave_words(bins, pl.lds.table_slots);
    threshold_row(a->thresholds[threshold], k.thr);
    const hipError_t le = ecdna::launch_pool_draws(k, st);
    const hipError_t se = hipStreamSynchronize(st);  // (also when the launch was refused: the uploads read the stack)
    TRY(le);
    TRY(se);
    if (out_thinned) TRY(to_host(out_thinned, reinterpret_cast<const uint64_t*>(d_thinned), thinned_words));
    if (out_kept) TRY(to_host(out_kept, reinterpret_cast<const uint64_t*>(d_kept), kept_words));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_rescored(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->kept.m) return fail(ECDNA_E_STATE, "download_rescored: the kept samples need ecdna_ssa_ctx_create_keep");
    if (!c->launched || !c->kept.valid)
        return fail(ECDNA_E_STATE, "download_rescored before rescore (a launch invalidates the rescored records)");
    return download_rescored_store(c, c->kept, out);
}

int ecdna_ssa_ctx_download_rescored_timepoints(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("download_rescored_timepoints") + kNeedsTimepoints);
    if (!c->launched || !c->kept_tp.valid)
        return fail(ECDNA_E_STATE, "download_rescored_timepoints before rescore_timepoints (a launch invalidates the "
                                   "rescored records; ecdna_ssa_ctx_create_keep_timepoints)");
    return download_rescored_store(c, c->kept_tp, out);
}

int ecdna_ssa_ctx_pool_accepted(ecdna_ssa_ctx* c, uint32_t threshold, uint64_t* out_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!out_hist) return fail(ECDNA_E_INVALID, "pool_accepted.out_hist is NULL");
    if (!c->kept.m) return fail(ECDNA_E_STATE, "pool_accepted: the kept samples need ecdna_ssa_ctx_create_keep");
    if (!c->launched || !c->accept_valid)
        return fail(ECDNA_E_STATE, "pool_accepted before accept (a launch invalidates the acceptance results)");
    if (threshold >= c->acc_rows)
        return fail(ECDNA_E_INVALID, "pool_accepted.threshold must be < n_thresholds of the last accept");
    return pool_store(c, c->kept, threshold, out_hist, "ecdna_ssa_ctx_pool_accepted");
}

int ecdna_ssa_ctx_pool_accepted_timepoints(ecdna_ssa_ctx* c, uint32_t threshold, uint64_t* out_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!out_hist) return fail(ECDNA_E_INVALID, "pool_accepted_timepoints.out_hist is NULL");
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("pool_accepted_timepoints") + kNeedsTimepoints);
    if (!c->launched || !c->accept_valid)
        return fail(ECDNA_E_STATE, "pool_accepted_timepoints before accept (a launch invalidates the acceptance results; "
                                   "ecdna_ssa_ctx_create_keep_timepoints)");
    if (threshold >= c->acc_rows)
        return fail(ECDNA_E_INVALID, "pool_accepted_timepoints.threshold must be < n_thresholds of the last accept");
    return pool_store(c, c->kept_tp, threshold, out_hist, "ecdna_ssa_ctx_pool_accepted_timepoints");
}

int ecdna_ssa_ctx_download_kept(ecdna_ssa_ctx* c, uint64_t n_ids, const uint64_t* ids, ecdna_kept_t* out_headers,
                                uint16_t* out_cells) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    std::vector<uint32_t> index(ids ? n_ids : 0);
    TRY(kept_index(c, "download_kept", n_ids, ids, index.data()));
    if (!c->kept.m) return fail(ECDNA_E_STATE, "download_kept: the kept samples need ecdna_ssa_ctx_create_keep");
    TRY(ctx_launched(c));
    return download_kept_store(c, c->kept, n_ids, ids ? index.data() : nullptr, out_headers, out_cells,
                               "ecdna_ssa_ctx_download_kept");
}

int ecdna_ssa_ctx_download_kept_timepoints(ecdna_ssa_ctx* c, uint64_t n_ids, const uint64_t* ids,
                                           ecdna_kept_t* out_headers, uint16_t* out_cells) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    std::vector<uint32_t> index(ids ? n_ids : 0);
    TRY(kept_index(c, "download_kept_timepoints", n_ids, ids, index.data()));
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("download_kept_timepoints") + kNeedsTimepoints);
    TRY(ctx_launched(c, "download_kept_timepoints before launch (ecdna_ssa_ctx_create_keep_timepoints)"));
    return download_kept_store(c, c->kept_tp, n_ids, ids ? index.data() : nullptr, out_headers, out_cells,
                               "ecdna_ssa_ctx_download_kept_timepoints");
}

int ecdna_ssa_ctx_select_digits(ecdna_ssa_ctx* c, uint32_t source, uint64_t timepoint_mask, uint32_t pass,
                                uint32_t n_prefixes, const uint64_t* prefixes, uint64_t* out_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (pass >= ecdna::select::kPasses) return fail(ECDNA_E_INVALID, "select_digits.pass must be in [0, 7]");
    if (n_prefixes < 1u || n_prefixes > ecdna::select::kMaxRanks)
        return fail(ECDNA_E_INVALID, "select_digits.n_prefixes must be in [1, 32]");
    if (!prefixes) return fail(ECDNA_E_INVALID, "select_digits.prefixes is NULL");
    if (!out_hist) return fail(ECDNA_E_INVALID, "select_digits.out_hist is NULL");
    SelectSource src;
    TRY(select_source(c, source, timepoint_mask, "select_digits", &src));
    return select_pass(c, source, src, pass, n_prefixes, prefixes, n_prefixes, out_hist, "ecdna_ssa_ctx_select_digits");
}

int ecdna_ssa_ctx_select(ecdna_ssa_ctx* c, const ecdna_ssa_select_t* s, uint64_t* out_population, uint64_t* out_ranks,
                         double* out_values, uint64_t* out_counts_le) {
    namespace sel = ecdna::select;
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!s) return fail(ECDNA_E_INVALID, "select is NULL");
    if (s->struct_size != sizeof(ecdna_ssa_select_t))
        return fail(ECDNA_E_INVALID, "select.struct_size must be sizeof(ecdna_ssa_select_t)");
    if (!is_accept_source(s->source))
        return fail(ECDNA_E_INVALID, "select.source is not an ecdna_accept_source_t");
    const uint32_t K = s->n_ranks;
    if (K < 1u || K > sel::kMaxRanks) return fail(ECDNA_E_INVALID, "select.n_ranks must be in [1, 32]");
    if ((s->ranks != nullptr) == (s->fractions != nullptr))
        return fail(ECDNA_E_INVALID, "exactly one of select.ranks and select.fractions must be given");
    for (uint32_t j = 0; j < K; ++j) {
        if (s->ranks && s->ranks[j] == 0u)
            return fail(ECDNA_E_INVALID, "select.ranks[" + std::to_string(j) + "] must be >= 1");
        if (s->fractions && !(s->fractions[j] > 0.0 && s->fractions[j] <= 1.0))
            return fail(ECDNA_E_INVALID, "select.fractions[" + std::to_string(j) + "] must be in (0, 1] and not NaN");
    }
    if (s->reserved) return fail(ECDNA_E_INVALID, "select.reserved must be 0");
    SelectSource src;
    TRY(select_source(c, s->source, s->timepoint_mask, "select", &src));

    sel::Walk walk;
    walk.start(K, s->ranks, s->fractions);
    std::vector<uint64_t> hist((uint64_t)sel::kDistances * K * sel::kDigits);
    for (uint32_t pass = 0; pass < sel::kPasses; ++pass) {
        TRY(select_pass(c, s->source, src, pass, K, walk.prefixes(), sel::kMaxRanks, hist.data(), "ecdna_ssa_ctx_select"));
        walk.feed(hist.data());
    }
    if (out_population) *out_population = walk.M;
    for (uint32_t j = 0; j < K; ++j) {
        if (out_ranks) out_ranks[j] = walk.rank[j];
        for (uint32_t x = 0; x < sel::kDistances; ++x) {
            if (out_values) out_values[(uint64_t)x * K + j] = walk.value(x, j);
            if (out_counts_le) out_counts_le[(uint64_t)x * K + j] = walk.counts_le(x, j);
        }
    }
    return ECDNA_OK;
}

// ---- the select over thinning draws (thinned select mapping v1): the keys of every (replicate, draw) of the block's
// range, made by the thinning core on buffers of its own, and ecdna_ssa_ctx_select's digit passes and walk over them ----

int ecdna_ssa_ctx_select_draws_digits(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t pass,
                                      uint32_t n_prefixes, const uint64_t* prefixes, uint64_t* out_hist) {
    namespace sd = ecdna::select_draws;
    namespace sel = ecdna::select;
    const char* who = "ecdna_ssa_ctx_select_draws_digits";
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    const std::string bad = sd::invalid_pass(pass, n_prefixes, prefixes, out_hist);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    KeptStore* s = nullptr;
    TRY(select_draws_store(c, a, &s));
    std::fill(out_hist, out_hist + (uint64_t)sel::kDistances * n_prefixes * sel::kDigits, 0ull);
    if (!c->p.n_replicates) return ECDNA_OK;
    TRY(hipSetDevice(c->device));
    if (pass == 0u) {
        TRY(select_draws_keys(c, *s, *a, who));
    } else if (!c->sdr_keys_valid || !sd::same(c->sdr_block, *a, c->p.hist_bins)) {
        return fail(ECDNA_E_STATE, "select_draws_digits: pass " + std::to_string(pass) +
                                       " has no keys to read: pass 0 of the same block must come first (a launch "
                                       "drops the keys)");
    }
    return select_draws_pass(c, a->n_draws, pass, n_prefixes, prefixes, n_prefixes, out_hist, who);
}

int ecdna_ssa_ctx_select_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t n_ranks,
                               const uint64_t* ranks, const double* fractions, uint64_t* out_population,
                               uint64_t* out_ranks, double* out_values, uint64_t* out_counts_le) {
    namespace sd = ecdna::select_draws;
    namespace sel = ecdna::select;
    const char* who = "ecdna_ssa_ctx_select_draws";
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    const std::string bad = sd::invalid_ranks(n_ranks, ranks, fractions);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    KeptStore* s = nullptr;
    TRY(select_draws_store(c, a, &s));
    const uint32_t K = n_ranks;
    const bool any = c->p.n_replicates != 0u;
    if (any) {
        TRY(hipSetDevice(c->device));
        TRY(select_draws_keys(c, *s, *a, who));
    }
    sel::Walk walk;
    walk.start(K, ranks, fractions);
    std::vector<uint64_t> hist((uint64_t)sel::kDistances * K * sel::kDigits, 0ull);
    for (uint32_t pass = 0; pass < sel::kPasses; ++pass) {
        if (any) TRY(select_draws_pass(c, a->n_draws, pass, K, walk.prefixes(), sel::kMaxRanks, hist.data(), who));
        walk.feed(hist.data());
    }
    if (out_population) *out_population = walk.M;
    for (uint32_t j = 0; j < K; ++j) {
        if (out_ranks) out_ranks[j] = walk.rank[j];
        for (uint32_t x = 0; x < sel::kDistances; ++x) {
            if (out_values) out_values[(uint64_t)x * K + j] = walk.value(x, j);
            if (out_counts_le) out_counts_le[(uint64_t)x * K + j] = walk.counts_le(x, j);
        }
    }
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_rng_words(ecdna_ssa_ctx* c, uint64_t* out) {
    TRY(ctx_launched(c));
    if (!c->d_rng_words) return fail(ECDNA_E_STATE, "stream positions need ECDNA_FLAG_REFERENCE_DRAWS");
    if (!out || !c->p.n_replicates) return ECDNA_OK;
    TRY(ctx_drain(c));
    TRY(to_host(out, c->d_rng_words, c->p.n_replicates));
    return ECDNA_OK;
}

int ecdna_ssa_ctx_destroy(ecdna_ssa_ctx* c) {
    free_ctx(c);
    return ECDNA_OK;
}

int ecdna_ssa_run(const ecdna_ssa_params_t* p, ecdna_rep_summary_t* out_summaries, uint64_t* out_hist,
                  ecdna_totals_t* out_totals, void* stream) {
    ecdna_ssa_ctx* c = nullptr;
    int rc = ecdna_ssa_ctx_create(p, &c);
    if (rc) return rc;
    rc = ecdna_ssa_ctx_launch(c, stream);
    if (!rc) rc = ecdna_ssa_ctx_download(c, out_summaries, out_hist, out_totals, nullptr);
    ecdna_ssa_ctx_destroy(c);
    return rc;
}

}  // extern "C"
