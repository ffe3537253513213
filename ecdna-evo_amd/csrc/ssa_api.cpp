// ssa_api.cpp — the C ABI of include/ecdna_ssa.h up to the end of a launch: parameter validation,
// device-resident run contexts, chunking by HBM capacity, launches of the
// stepper and end-of-run kernels (ssa_kernels.hip, ssa_hist.hip, ssa_subsample.hip, ssa_snapstats.hip,
// ssa_passage.hip, ssa_cohort.hip, and the keep passes into the kept-sample stores), the run's own downloads, and the
// library's error message. The context itself is ssa_ctx.hpp's; the passes that run after a launch (acceptance, select,
// and everything over the kept samples) are ssa_api_passes.cpp's. Everything that decides the stepper's launch is here.
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
#include "ssa_cohort.hpp"
#include "ssa_ctx.hpp"
#include "ssa_keep.hpp"
#include "ssa_launch.h"
#include "ssa_plan.hpp"

using namespace ecdna::api;

namespace {
thread_local std::string g_last_error;
}

int ecdna::api::fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

namespace {

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
    delete c;  // (the post-run passes' buffers free themselves, on the device set above)
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

// ---- ecdna_ssa_ctx_create_cohort, step by step (build_ctx has the order: the chunk size depends on what is allocated
// before gather_facts asks for the free memory) ----

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

uint32_t pass_blocks(const ecdna::ChunkIds& ids) { return (ids.n + ids.reps_per_block - 1) / ids.reps_per_block; }

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

}  // namespace

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
    c->on_launch();  // (what the post-run passes hold was made from the previous launch's records and kept samples)
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
