// ssa_ctx.hpp — what the translation units of the C ABI share (ssa_api.cpp: create, plan, launch and the run's own
// downloads; ssa_api_passes.cpp: the passes that run after a launch; ssa_comm.cpp: the reduction): the error channel,
// the run context with its device buffers, the kept-sample stores and one state struct per post-run pass, and the small
// helpers every unit calls. Library-internal: everything here has hidden visibility, so nothing of it is in the
// library's dynamic symbol table.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/ecdna_ssa.h"
#include "ssa_accept_draws.hpp"
#include "ssa_cohort.hpp"
#include "ssa_launch.h"
#include "ssa_plan.hpp"
#include "ssa_select_draws.hpp"

#pragma GCC visibility push(hidden)

namespace ecdna {
namespace api {

// Records the calling thread's error message and returns `code` (ssa_api.cpp holds the message).
int fail(int code, const std::string& msg);

// TRY(expr): return from the calling function with the error of a failed step, which is either a HIP call (the
// error is recorded here, with the call's text) or a function of the library that returns an ECDNA_* code (and has
// recorded its own).
inline int rc_of(int rc, const char*) { return rc; }
inline int rc_of(hipError_t e, const char* what) {
    if (e == hipSuccess) return ECDNA_OK;
    return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define TRY(expr)                                                     \
    do {                                                              \
        if (int _rc = ::ecdna::api::rc_of((expr), #expr)) return _rc; \
    } while (0)

// The index of the first of `count` target histograms ([count][bins]) without a cell; count if there is none, or no
// targets at all.
inline uint32_t first_empty_target(const uint64_t* hists, uint32_t count, uint32_t bins) {
    for (uint32_t i = 0; hists && i < count; ++i) {
        const uint64_t* t = hists + (uint64_t)i * bins;
        if (std::all_of(t, t + bins, [](uint64_t x) { return x == 0; })) return i;
    }
    return count;
}

// The step between the global ids of a call's replicates (replicate_stride = 0 stands for 1).
inline uint64_t rid_stride(const ecdna_ssa_params_t& p) { return p.replicate_stride ? p.replicate_stride : 1u; }

// The Philox key of growth phase g of a passage run (passage mapping v1, include/ecdna_ssa.h): the seed itself for
// phase 0, else the splitmix64 finaliser of seed + g * 0x9E3779B97F4A7C15.
inline uint64_t passage_seed(uint64_t seed, uint32_t g) {
    if (g == 0) return seed;
    uint64_t z = seed + (uint64_t)g * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Sum of a target histogram (> 0 for a usable target), and for `count` of them ([count][bins]) what the kernels
// compare against: the CDFs over the bins ([count][bins]) and the scalars ([count][3]: mean, entropy, N+ frequency;
// the overflow bin counts at k = bins - 1).
inline double target_total(const uint64_t* hist, uint32_t bins) {
    double tot = 0.0;
    for (uint32_t b = 0; b < bins; ++b) tot += (double)hist[b];
    return tot;
}
inline void summarize_targets(const uint64_t* hists, uint64_t count, uint32_t bins, double* out_cdf,
                              double* out_scalars) {
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

// `count` elements from the device to the host, and from device to device on a stream.
template <typename T>
hipError_t to_host(T* out, const T* dev, uint64_t count) {
    return hipMemcpy(out, dev, count * sizeof(T), hipMemcpyDeviceToHost);
}
template <typename T>
hipError_t copy_async(T* dst, const T* src, uint64_t count, hipStream_t st) {
    return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, st);
}

// A chunk as planned (first, n, its grid, rotation's partition size, the drain control), and what the context adds.
struct Chunk : plan::ChunkPlan {
    std::vector<hipEvent_t> ev;  // per growth phase (one in an ordinary run): start, stepper done, passes done
    std::vector<RotPart> rot_init;  // replicate rotation (rot_n_pad > 0): the counters it starts from
};

// A device buffer of a post-run pass: it belongs to the context but not to `owned`, as it is allocated at the first
// call that needs it and replaced by a larger one when a later call needs more. Freed with its owner.
struct DeviceBuf {
    void* ptr = nullptr;
    uint64_t bytes = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() {
        if (ptr) (void)hipFree(ptr);
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(ptr);
    }
    // At least `need` bytes. A larger buffer is allocated before the old one is freed (hipFree waits for the device, so
    // an earlier pass that still writes the old one has finished): a failure leaves the buffer as it was. what, who:
    // the buffer and the calling entry point, for the message.
    int reserve(uint64_t need, const char* what, const char* who) {
        if (need <= bytes) return ECDNA_OK;
        void* fresh = nullptr;
        const hipError_t e = hipMalloc(&fresh, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();  // (the context stays usable)
            return fail(e == hipErrorOutOfMemory ? ECDNA_E_NOMEM : ECDNA_E_HIP,
                        std::string(who) + ": the " + what + " buffer (" + std::to_string(need) +
                            " bytes) does not fit: " + hipGetErrorString(e));
        }
        if (ptr) (void)hipFree(ptr);
        ptr = fresh;
        bytes = need;
        return ECDNA_OK;
    }
};

// The targets of one call on the device: their CDFs [P][bins] and scalars [P][3], and the host copies the two uploads
// read, which therefore live here and not on a stack. `pending`: uploads (and the pass that reads the device copies)
// were enqueued on `stream` since it was last drained; every call drains before it replaces either copy. (The host
// copies are declared first, so at destroy the buffers are freed, which waits for the device, before they go.)
struct TargetSet {
    std::vector<double> host_cdf, host_scalars;
    DeviceBuf cdf, scalars;
    bool pending = false;
    hipStream_t stream = nullptr;

    // Waits for what is pending.
    int drain() {
        if (pending) TRY(hipStreamSynchronize(stream));
        pending = false;
        return ECDNA_OK;
    }
    // Device room for P targets of `bins` bins. who: the calling entry point, for the message.
    int reserve(uint64_t P, uint32_t bins, const char* who) {
        TRY(cdf.reserve(P * bins * sizeof(double), "target CDFs", who));
        TRY(scalars.reserve(P * 3u * sizeof(double), "target scalars", who));
        return ECDNA_OK;
    }
    // The targets' CDFs and scalars (summarize_targets) into the host copies, and their two uploads enqueued on st.
    // `pending` is set before the first: a failure between the two is drained by the next call, or by destroy.
    int upload(const uint64_t* target_hists, uint64_t P, uint32_t bins, hipStream_t st) {
        host_cdf.resize(P * bins);
        host_scalars.resize(P * 3u);
        summarize_targets(target_hists, P, bins, host_cdf.data(), host_scalars.data());
        pending = true;
        stream = st;
        TRY(hipMemcpyAsync(cdf.ptr, host_cdf.data(), host_cdf.size() * sizeof(double), hipMemcpyHostToDevice, st));
        TRY(hipMemcpyAsync(scalars.ptr, host_scalars.data(), host_scalars.size() * sizeof(double),
                           hipMemcpyHostToDevice, st));
        return ECDNA_OK;
    }
};

// A store of kept samples (m = 0: the context has no such block): the keep block's (ecdna_ssa_keep_t), one slice, or the
// timepoint keep block's (ecdna_ssa_keep_timepoints_t), a slice per timepoint — the run's snapshots or growth phases.
// Headers [T][n] and cells [T][n][m] are sized by the run and written by the keep pass of every chunk. The store's last
// rescore left its records [T][P][n] and the targets they were scored against ([T][P] of them).
struct KeptStore {
    uint32_t m = 0, T = 0;
    uint2* d_headers = nullptr;
    uint16_t* d_cells = nullptr;
    DeviceBuf stats;
    TargetSet scored;
    bool valid = false;    // (a launch invalidates the records)
    uint32_t targets = 0;  // the P of the last rescore: targets per slice (the timepoint keep block: 1)
    void on_launch() { valid = false; }
    // Slice t of a run of n replicates: a run of kept samples as the keep block's.
    struct Slice {
        uint2* headers;
        uint16_t* cells;
    };
    Slice slice(uint64_t t, uint64_t n) const { return {d_headers + t * n, d_cells + t * n * m}; }
};

// ---- one state per post-run pass: its buffers, what its last call left, and what a launch does to it ----

// ecdna_ssa_ctx_accept: mask [n] u32, counts [Q][n_sets] u64, workgroup counts, and the list's ids [cap] and records
// [cap][T]; what the last call left for ecdna_ssa_ctx_download_accept.
struct AcceptState {
    DeviceBuf mask, counts, blocks, ids, list;
    bool valid = false;
    uint32_t rows = 0, timepoints = 0, list_row = 0;
    uint64_t list_cap = 0;  // entries of the device list: min(list_capacity, n_replicates)
    void on_launch() { valid = false; }  // (the results were the previous launch's)
};
// ecdna_ssa_ctx_select / _select_digits: the keys [4][n] u64 of one (source, timepoint mask), kept between passes and
// calls until the records they were made from are replaced, and one pass's histogram [4][kMaxSelectGroups][256] u64.
struct SelectState {
    DeviceBuf keys, hist;
    bool keys_valid = false;
    uint32_t source = 0;
    uint64_t tmask = 0;
    void on_launch() { keys_valid = false; }
};
// What the passes over either store share (both are synchronous): the pooled histogram [T][sets][bins] of
// _pool_accepted, and the gather's index [n_ids] and staging [T][n_ids] of _download_kept. No result is held.
struct StoreScratch {
    DeviceBuf pool_hist, gat_index, gat_headers, gat_cells;
    void on_launch() {}
};
// ecdna_ssa_ctx_accept_draws: the call's own targets, passes [n][Q] u8 and sums [Q][n_sets] u64; what the last call
// left for ecdna_ssa_ctx_download_accept_draws.
struct AcceptDrawsState {
    TargetSet targets;
    DeviceBuf passes, sums;
    bool valid = false;
    uint32_t rows = 0;
    void on_launch() { valid = false; }
};
// ecdna_ssa_ctx_pool_draws: the call's own targets, and its pooled arrays, thinned [targets][sets][bins] then kept
// [slices][sets][bins] u64. The call is synchronous and holds no result.
struct PoolDrawsState {
    TargetSet targets;
    DeviceBuf pool;
    void on_launch() {}
};
// ecdna_ssa_ctx_select_draws / _select_draws_digits: the call's own targets, its keys [4][n x n_draws] u64 and one
// pass's histogram; the block the keys were made for, kept between the passes of _select_draws_digits until a launch
// replaces the kept samples they were made from.
struct SelectDrawsState {
    TargetSet targets;
    DeviceBuf keys, hist;
    bool keys_valid = false;
    select_draws::Block block;
    void on_launch() { keys_valid = false; }
};

}  // namespace api
}  // namespace ecdna

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
    std::vector<ecdna::api::Chunk> chunks;
    bool launched = false;
    // the kept samples: the keep block's store (ecdna_ssa_ctx_rescore's records [P][n]) and the timepoint keep block's
    // (ecdna_ssa_ctx_rescore_timepoints's [T][n]), each with its own records, targets and validity
    ecdna::api::KeptStore kept, kept_tp;
    // the post-run passes (ssa_api_passes.cpp): each one's buffers free themselves with the context
    ecdna::api::AcceptState acc;
    ecdna::api::SelectState sel;
    ecdna::api::StoreScratch scratch;
    ecdna::api::AcceptDrawsState adr;
    ecdna::api::PoolDrawsState pdr;
    ecdna::api::SelectDrawsState sdr;
    // A launch replaces what every pass's results were made from.
    void on_launch() {
        kept.on_launch();
        kept_tp.on_launch();
        acc.on_launch();
        sel.on_launch();
        scratch.on_launch();
        adr.on_launch();
        pdr.on_launch();
        sdr.on_launch();
    }
};

namespace ecdna {
namespace api {

// The preludes of the sync and download functions: a context that was launched; its device current and its stream
// drained. (Between the two a download checks what else it needs, and returns early when there is nothing to copy.)
inline int ctx_launched(const ecdna_ssa_ctx* c, const char* what = "download before launch") {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched) return fail(ECDNA_E_STATE, what);
    return ECDNA_OK;
}
inline int ctx_drain(ecdna_ssa_ctx* c) {
    TRY(hipSetDevice(c->device));
    TRY(hipStreamSynchronize(c->last_stream));
    return ECDNA_OK;
}

// A workgroup's share of the chunk's n replicates in an end-of-run pass: the chunk over eight workgroups per CU, at
// least `floor`. (Eight per CU for either histogram pass: one per CU made the bin store's lane-per-replicate pass no
// faster at C3, 0.29 -> 0.30 ms, and C4's 1,024 sets 5 -> 28 ms, each workgroup walking more sets. The sampling
// passes run one wave per population: at least one per wave of the workgroup, at most the histogram pass's share,
// which bounds the sets a workgroup walks.)
inline uint32_t pass_reps_per_block(const ecdna_ssa_ctx* c, uint32_t n, uint32_t floor) {
    const uint32_t hist_blocks_max = (uint32_t)c->cus * 8u;
    return std::max<uint32_t>(floor, (n + hist_blocks_max - 1) / hist_blocks_max);
}
// The share of a pass that sums histograms per parameter set, in workgroups of `block` lanes (the histogram pass, and
// the pooling of the kept samples): at least one replicate per lane of a workgroup, or the chunk's replicates of one
// parameter set if fewer: small runs otherwise spread over 2,048 workgroups of mostly idle waves, each adding its own
// nonzero bins to the same global words (C2: 0.061 -> 0.023 ms per launch at 256, 0.038 at 64, 0.052 at 1,024;
// profiles/r06ak_hist_rpb.txt); sweeps of small sets keep about one set per workgroup
inline uint32_t hist_reps_per_block(const ecdna_ssa_ctx* c, uint32_t n, uint32_t block) {
    const uint64_t set_local = c->p.reps_per_set / rid_stride(c->p);
    return pass_reps_per_block(c, n, (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(block, set_local)));
}

}  // namespace api
}  // namespace ecdna

#pragma GCC visibility pop
