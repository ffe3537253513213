// ssa_api_passes.cpp — the part of the C ABI of include/ecdna_ssa.h that runs after a launch: the acceptance pass
// (ssa_accept.hip), the radix select of its thresholds (ssa_select.hip), and the passes over the kept samples
// (ssa_rescore.hip, ssa_thin.hip, ssa_accept_draws.hip, ssa_pool_draws.hip, ssa_select_draws.hip). Each pass keeps its
// buffers and what its last call left in a state struct of the context (ssa_ctx.hpp), which a launch resets through
// ecdna_ssa_ctx::on_launch. The kept samples of the keep block and of the timepoint keep block lie in one kind of store
// (KeptStore), and every pass over them has one implementation, which the two blocks' entry points call.
//
// Nothing here decides the stepper's launch: creation, the launch plan, the launch and the run's own downloads are
// ssa_api.cpp's. Everything here is host code; there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ecdna_ssa.h"
#include "ssa_accept_draws.hpp"
#include "ssa_ctx.hpp"
#include "ssa_keep.hpp"
#include "ssa_launch.h"
#include "ssa_pool_draws.hpp"
#include "ssa_select.hpp"
#include "ssa_select_draws.hpp"
#include "ssa_thin.hpp"

using namespace ecdna::api;

namespace {

// ---- ecdna_ssa_ctx_accept: the source's records on the device and how they lie, then the pass's own buffers ----

// What an ecdna_accept_source_t names in this context (ssa_launch.h AcceptArgs has the strides' meaning); ECDNA_E_STATE
// under the conditions of the matching download.
// Whether a number names a source: the one predicate of ecdna_ssa_ctx_accept, checked_source and ecdna_ssa_ctx_select (6
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
            s.stats = c->kept.stats.as<const ecdna_rep_stats_t>();
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
            s.stats = c->kept_tp.stats.as<const ecdna_rep_stats_t>();
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

// The source's records and the participating timepoints: what ecdna_ssa_ctx_accept, _select and _select_digits check
// after their own arguments, in this order. who: "accept", "select" or "select_digits", the prefix of the messages' field
// names; untold: what scores without a target cannot tell, the tail of that message.
struct CheckedSource {
    AcceptSource src;
    uint64_t tmask = 0;
};
int checked_source(const ecdna_ssa_ctx* c, uint32_t source, uint64_t timepoint_mask, const std::string& who,
                   const char* untold, CheckedSource* out) {
    if (!is_accept_source(source))
        return fail(ECDNA_E_INVALID, who + ".source is not an ecdna_accept_source_t");
    if (c->p.n_replicates >= (1ull << 32)) return fail(ECDNA_E_INVALID, who + ": n_replicates must be < 2^32");
    TRY(accept_source(c, source, &out->src));
    const uint32_t T = out->src.T;
    const std::string bad = ecdna::accept_draws::invalid_timepoint_mask(who, timepoint_mask, T);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    TRY(ctx_launched(c, (who + " before launch").c_str()));
    if (!out->src.has_target)
        return fail(ECDNA_E_STATE, who + ": the source's statistics were computed without a target (every distance is "
                                         "0: " + untold + ")");
    out->tmask = timepoint_mask ? timepoint_mask : ecdna::accept_draws::all_timepoints(T);
    return ECDNA_OK;
}
const char* const kNoQuantile = "no quantile tells replicates apart";

// A threshold row as the kernels' argument blocks carry it.
void threshold_row(const ecdna_accept_threshold_t& t, double* row) {
    row[0] = t.ks;
    row[1] = t.mean_rel;
    row[2] = t.entropy_rel;
    row[3] = t.frequency_diff;
}

// ---- ecdna_ssa_ctx_select / _select_digits: one digit pass ----

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
int select_pass(ecdna_ssa_ctx* c, uint32_t source, const CheckedSource& s, uint32_t pass, uint32_t K,
                const uint64_t* prefixes, uint32_t stride, uint64_t* out_hist, const char* who) {
    namespace sel = ecdna::select;
    const uint64_t n = c->p.n_replicates;
    SelectState& my = c->sel;
    std::fill(out_hist, out_hist + (uint64_t)sel::kDistances * K * sel::kDigits, 0ull);
    if (!n) return ECDNA_OK;
    TRY(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    const bool cached = my.keys_valid && my.source == source && my.tmask == s.tmask;
    if (!cached) {
        my.keys_valid = false;
        TRY(my.keys.reserve(sel::kDistances * n * sizeof(uint64_t), "keys", who));
    }
    TRY(my.hist.reserve(kSelectHistWords * sizeof(uint64_t), "histogram", who));
    if (!cached) {
        ecdna::SelectKeyArgs k{};
        k.stats = s.src.stats;
        k.summaries = s.src.summaries;
        k.rep_stride = s.src.rep_stride;
        k.tp_stride = s.src.tp_stride;
        k.err_stride = s.src.err_stride;
        k.tmask = s.tmask;
        k.keys = my.keys.as<uint64_t>();
        k.n = (uint32_t)n;
        k.T = s.src.T;
        TRY(ecdna::launch_select_keys(k, st));
        my.source = source;
        my.tmask = s.tmask;
        my.keys_valid = true;
    }
    return digit_pass(my.keys.as<const uint64_t>(), (uint32_t)n, my.hist.ptr, pass, K, prefixes, stride, out_hist, st);
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
    TRY(s->scored.drain());
    s->valid = false;
    c->sel.on_launch();  // (the select passes' keys may have been made from the records this call replaces)
    TRY(s->stats.reserve(std::max<uint64_t>(n, 1) * targets * sizeof(ecdna_rep_stats_t), "records", who));
    TRY(s->scored.reserve(targets, bins, who));
    if (n) {
        TRY(s->scored.upload(target_hists, targets, bins, st));
        // slice t's part of the store, the same for either pass (RescoreArgs' fields, which ThinArgs repeats)
        auto slice = [&](auto a, uint64_t t) {
            const KeptStore::Slice at = s->slice(t, n);
            a.headers = at.headers;
            a.cells = at.cells;
            a.out = s->stats.as<ecdna_rep_stats_t>() + t * P * n;
            a.target_cdf = s->scored.cdf.as<const double>() + t * P * bins;
            a.target_scalars = s->scored.scalars.as<const double>() + t * P * 3u;
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
    if (out && records) TRY(to_host(out, s.stats.as<const ecdna_rep_stats_t>(), records));
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
    DeviceBuf& pool = c->scratch.pool_hist;
    TRY(pool.reserve(T * nb * sizeof(uint64_t), "histogram", who));
    TRY(hipMemsetAsync(pool.ptr, 0, T * nb * sizeof(uint64_t), st));
    for (uint64_t t = 0; t < T; ++t) {
        const KeptStore::Slice at = s.slice(t, n);
        ecdna::PoolAcceptedArgs a{};
        a.headers = at.headers;
        a.cells = at.cells;
        a.mask = c->acc.mask.as<const uint32_t>();
        a.hist = pool.as<unsigned long long>() + t * nb;
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
    TRY(to_host(out_hist, pool.as<const uint64_t>(), T * nb));
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
        StoreScratch& g = c->scratch;
        TRY(g.gat_index.reserve(n_ids * sizeof(uint32_t), "index", who));
        TRY(g.gat_headers.reserve(T * n_ids * sizeof(uint2), "headers", who));
        TRY(g.gat_cells.reserve(T * n_ids * m * sizeof(uint16_t), "cells", who));
        hipStream_t st = c->last_stream;
        TRY(hipMemcpy(g.gat_index.ptr, index, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice));
        for (uint64_t t = 0; t < T; ++t) {
            const KeptStore::Slice at = s.slice(t, n);
            ecdna::KeptGatherArgs a{};
            a.headers = at.headers;
            a.cells = at.cells;
            a.index = g.gat_index.as<const uint32_t>();
            a.out_headers = g.gat_headers.as<uint2>() + t * n_ids;
            a.out_cells = g.gat_cells.as<uint16_t>() + t * n_ids * m;
            a.n_ids = (uint32_t)n_ids;
            a.m = (uint32_t)m;
            TRY(ecdna::launch_kept_gather(a, st));
        }
        TRY(hipStreamSynchronize(st));
        if (out_headers)
            TRY(hipMemcpy(out_headers, g.gat_headers.ptr, T * n_ids * sizeof(uint2), hipMemcpyDeviceToHost));
        if (out_cells) TRY(to_host(out_cells, g.gat_cells.as<const uint16_t>(), T * n_ids * m));
        return ECDNA_OK;
    }
    for (uint64_t t = 0; t < T; ++t) {
        const KeptStore::Slice at = s.slice(t, n);
        if (out_headers)
            TRY(hipMemcpy(out_headers + t * n_ids, at.headers, n_ids * sizeof(uint2), hipMemcpyDeviceToHost));
        if (out_cells) TRY(to_host(out_cells + t * n_ids * m, static_cast<const uint16_t*>(at.cells), n_ids * m));
    }
    return ECDNA_OK;
}

const char* const kNeedsTimepoints = ": the kept timepoint samples need ecdna_ssa_ctx_create_keep_timepoints";

// ---- ecdna_ssa_ctx_accept_draws, _pool_draws and _select_draws: what they do with the block they share ----

// The store the block names, under the checks the calls make and in their order. name: "accept_draws", "pool_draws" or
// "select_draws", the prefix of the messages; invalid(keep_cells): the call's own validation (accept_draws::invalid,
// pool_draws::invalid, select_draws::invalid).
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

// The part of the argument block the passes share, for the block's draws on store s: its slices and the mask are the
// plan's (accept_draws::plan), the LDS plan the call's, the targets the call's own device copies.
ecdna::DrawsArgs draws_args(const ecdna_ssa_ctx* c, const KeptStore& s, const ecdna_ssa_accept_draws_t& a,
                            const ecdna::accept_draws::Plan& slices, const ecdna::thin::LdsPlan& lds,
                            const TargetSet& targets) {
    const ecdna_ssa_params_t& p = c->p;
    const bool phases = &s == &c->kept_tp && c->n_passages;
    ecdna::DrawsArgs k{};
    k.headers = s.d_headers;
    k.cells = s.d_cells;
    // rule 1 as the sources 12 and 13 have it: the one summary, or on a passage context every participating phase's
    k.summaries = phases ? c->d_pas_summ : c->d_summ;
    k.err_stride = phases ? p.n_replicates : 0u;
    k.target_cdf = targets.cdf.as<const double>();
    k.target_scalars = targets.scalars.as<const double>();
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

// ---- ecdna_ssa_ctx_select_draws / _select_draws_digits: what both do after their own argument checks ----

// The store of the block and the state checks, as draws_store makes them under select_draws::invalid.
int select_draws_store(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, KeptStore** out) {
    return draws_store(c, a, "select_draws", [&](uint32_t keep_cells) {
        return ecdna::select_draws::invalid(c->p.hist_bins, keep_cells, c->kept_tp.T, c->p.n_replicates, *a);
    }, out);
}

// The keys of every (replicate, draw) of the block, into the context's buffer, which it then holds for that block.
// n > 0. Synchronises.
int select_draws_keys(ecdna_ssa_ctx* c, const KeptStore& s, const ecdna_ssa_accept_draws_t& a, const char* who) {
    namespace sd = ecdna::select_draws;
    const uint32_t bins = c->p.hist_bins, P = a.n_targets;
    hipStream_t st = c->last_stream;
    SelectDrawsState& my = c->sdr;
    my.keys_valid = false;
    TRY(my.targets.drain());
    TRY(my.targets.reserve(P, bins, who));
    TRY(my.keys.reserve(sd::keys_bytes(c->p.n_replicates, a.n_draws), "keys", who));
    TRY(my.targets.upload(a.target_hists, P, bins, st));
    const ecdna::accept_draws::Plan pl =
        ecdna::accept_draws::plan(bins, s.m, a.timepoints == 1u, P, a.sample_cells, a.timepoint_mask);
    ecdna::SelectDrawsArgs k{};
    k.s = draws_args(c, s, a, pl, pl.lds, my.targets);
    k.g = pl.grouping();
    k.keys = my.keys.as<uint64_t>();
    const hipError_t le = ecdna::launch_select_draws_keys(k, st);
    const int se = my.targets.drain();  // (also when the launch was refused: the call is synchronous on every path)
    TRY(le);
    TRY(se);
    my.block = sd::remember(a, bins);
    my.keys_valid = true;
    return ECDNA_OK;
}

// One digit pass over the keys select_draws_keys made.
int select_draws_pass(ecdna_ssa_ctx* c, uint32_t n_draws, uint32_t pass, uint32_t K, const uint64_t* prefixes,
                      uint32_t stride, uint64_t* out_hist, const char* who) {
    TRY(c->sdr.hist.reserve(ecdna::select_draws::hist_bytes(), "histogram", who));
    return digit_pass(c->sdr.keys.as<const uint64_t>(),
                      (uint32_t)ecdna::select_draws::n_keys(c->p.n_replicates, n_draws), c->sdr.hist.ptr, pass, K,
                      prefixes, stride, out_hist, c->last_stream);
}
}  // namespace

extern "C" {

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
    const std::string bad = ecdna::accept_draws::invalid_threshold_rows("accept", a->n_thresholds, a->thresholds);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    if (a->reserved) return fail(ECDNA_E_INVALID, "accept.reserved must be 0");
    CheckedSource cs;
    TRY(checked_source(c, a->source, a->timepoint_mask, "accept", "nothing could be rejected", &cs));
    const AcceptSource& src = cs.src;

    const char* who = "ecdna_ssa_ctx_accept";
    const ecdna_ssa_params_t& p = c->p;
    const uint64_t n = p.n_replicates;
    const uint32_t Q = a->n_thresholds;
    const uint64_t list_cap = std::min<uint64_t>(a->list_capacity, n);
    const uint32_t n_blocks = (uint32_t)((n + ecdna::kAcceptBlock - 1) / ecdna::kAcceptBlock);
    AcceptState& my = c->acc;
    my.valid = false;
    TRY(hipSetDevice(c->device));
    TRY(my.counts.reserve((uint64_t)Q * p.n_param_sets * sizeof(uint64_t), "counts", who));
    if (n) TRY(my.mask.reserve(n * sizeof(uint32_t), "mask", who));
    if (list_cap) {
        TRY(my.blocks.reserve((uint64_t)n_blocks * sizeof(uint32_t), "workgroup counts", who));
        TRY(my.ids.reserve(list_cap * sizeof(uint64_t), "list ids", who));
        TRY(my.list.reserve(list_cap * src.T * sizeof(ecdna_rep_stats_t), "list records", who));
    }

    hipStream_t st = c->last_stream;
    TRY(hipMemsetAsync(my.counts.ptr, 0, (uint64_t)Q * p.n_param_sets * sizeof(uint64_t), st));
    if (n) {
        ecdna::AcceptArgs k{};
        k.stats = src.stats;
        k.summaries = src.summaries;
        k.rep_stride = src.rep_stride;
        k.tp_stride = src.tp_stride;
        k.err_stride = src.err_stride;
        k.tmask = cs.tmask;
        k.rid0 = p.first_replicate;
        k.rid_stride = rid_stride(p);
        k.reps_per_set = p.reps_per_set;
        k.n = (uint32_t)n;
        k.T = src.T;
        k.Q = Q;
        k.n_sets = p.n_param_sets;
        k.mask = my.mask.as<uint32_t>();
        k.counts = my.counts.as<unsigned long long>();
        k.list_q = a->list_threshold;
        k.n_blocks = n_blocks;
        k.block_counts = my.blocks.as<uint32_t>();
        k.list_capacity = list_cap;
        k.ids = my.ids.as<uint64_t>();
        k.list_stats = my.list.as<ecdna_rep_stats_t>();
        for (uint32_t q = 0; q < Q; ++q) threshold_row(a->thresholds[q], k.thr[q]);
        TRY(ecdna::launch_accept_mask(k, st));
        if (list_cap) TRY(ecdna::launch_accept_list(k, st));
    }
    my.rows = Q;
    my.timepoints = src.T;
    my.list_row = a->list_threshold;
    my.list_cap = list_cap;
    my.valid = true;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_accept(ecdna_ssa_ctx* c, uint64_t* out_counts, uint32_t* out_mask,
                                  uint64_t* out_n_accepted, uint64_t* out_ids,
                                  ecdna_rep_stats_t* out_list_stats) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched || !c->acc.valid)
        return fail(ECDNA_E_STATE, "download_accept before accept (a launch invalidates the acceptance results)");
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const AcceptState& my = c->acc;
    const uint64_t* d_counts = my.counts.as<const uint64_t>();
    // the number accepted under the list's row: the sum of its counts over the sets
    std::vector<uint64_t> row(p.n_param_sets);
    TRY(to_host(row.data(), d_counts + (uint64_t)my.list_row * p.n_param_sets, p.n_param_sets));
    uint64_t n_accepted = 0;
    for (const uint64_t x : row) n_accepted += x;
    if (out_n_accepted) *out_n_accepted = n_accepted;
    if (out_counts) TRY(to_host(out_counts, d_counts, (uint64_t)my.rows * p.n_param_sets));
    if (out_mask && p.n_replicates) TRY(to_host(out_mask, my.mask.as<const uint32_t>(), p.n_replicates));
    const uint64_t listed = std::min<uint64_t>(n_accepted, my.list_cap);
    if (out_ids && listed) TRY(to_host(out_ids, my.ids.as<const uint64_t>(), listed));
    if (out_list_stats && listed)
        TRY(to_host(out_list_stats, my.list.as<const ecdna_rep_stats_t>(), listed * my.timepoints));
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
    AcceptDrawsState& my = c->adr;
    // an earlier call may still read the targets this one replaces (and its upload their host copies)
    TRY(my.targets.drain());
    my.valid = false;
    TRY(my.targets.reserve(P, bins, who));
    TRY(my.sums.reserve(ad::sums_bytes(Q, p.n_param_sets), "sums", who));
    if (n) TRY(my.passes.reserve(ad::passes_bytes(n, Q), "passes", who));
    TRY(hipMemsetAsync(my.sums.ptr, 0, ad::sums_bytes(Q, p.n_param_sets), st));
    if (n) {
        TRY(my.targets.upload(a->target_hists, P, bins, st));  // (the call only enqueues)
        const ad::Plan pl = ad::plan(bins, s->m, a->timepoints == 1u, P, a->sample_cells, a->timepoint_mask);
        ecdna::AcceptDrawsArgs k{};
        k.s = draws_args(c, *s, *a, pl, pl.lds, my.targets);
        k.g = pl.grouping();
        k.passes = my.passes.as<uint8_t>();
        k.sums = my.sums.as<unsigned long long>();
        k.Q = Q;
        for (uint32_t q = 0; q < Q; ++q) threshold_row(a->thresholds[q], k.thr[q]);
        TRY(ecdna::launch_accept_draws(k, st));
    }
    my.rows = Q;
    my.valid = true;
    return ECDNA_OK;
}

int ecdna_ssa_ctx_download_accept_draws(ecdna_ssa_ctx* c, uint64_t* out_sums, uint8_t* out_passes) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!c->launched || !c->adr.valid)
        return fail(ECDNA_E_STATE, "download_accept_draws before accept_draws (a launch invalidates its results)");
    TRY(ctx_drain(c));
    const ecdna_ssa_params_t& p = c->p;
    const AcceptDrawsState& my = c->adr;
    if (out_sums) TRY(to_host(out_sums, my.sums.as<const uint64_t>(), (uint64_t)my.rows * p.n_param_sets));
    if (out_passes && p.n_replicates)
        TRY(to_host(out_passes, my.passes.as<const uint8_t>(), p.n_replicates * my.rows));
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
    PoolDrawsState& my = c->pdr;
    TRY(my.targets.drain());
    TRY(my.targets.reserve(P, bins, who));
    TRY(my.pool.reserve(pd::pooled_bytes(P, S, sets, bins), "pooled histograms", who));
    unsigned long long* d_thinned = my.pool.as<unsigned long long>();
    unsigned long long* d_kept = d_thinned + thinned_words;
    TRY(hipMemsetAsync(my.pool.ptr, 0, pd::pooled_bytes(P, S, sets, bins), st));
    TRY(my.targets.upload(a->target_hists, P, bins, st));

    ecdna::PoolDrawsArgs k{};
    // (the slices and the mask are the verdict's: the pooling grouping walks every slice whatever the mask)
    k.s = draws_args(c, *s, *a, pl.verdict, pl.lds, my.targets);
    k.verdict = pl.verdict.grouping();
    k.pool = pl.pool.grouping();
    k.thinned = out_thinned ? d_thinned : nullptr;
    k.kept = out_kept ? d_kept : nullptr;
    k.wave_words = ecdna::pool_draws_wave_words(bins, pl.lds.table_slots);
    threshold_row(a->thresholds[threshold], k.thr);
    const hipError_t le = ecdna::launch_pool_draws(k, st);
    const int se = my.targets.drain();  // (also when the launch was refused: the call is synchronous on every path)
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
    if (!c->launched || !c->acc.valid)
        return fail(ECDNA_E_STATE, "pool_accepted before accept (a launch invalidates the acceptance results)");
    if (threshold >= c->acc.rows)
        return fail(ECDNA_E_INVALID, "pool_accepted.threshold must be < n_thresholds of the last accept");
    return pool_store(c, c->kept, threshold, out_hist, "ecdna_ssa_ctx_pool_accepted");
}

int ecdna_ssa_ctx_pool_accepted_timepoints(ecdna_ssa_ctx* c, uint32_t threshold, uint64_t* out_hist) {
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    if (!out_hist) return fail(ECDNA_E_INVALID, "pool_accepted_timepoints.out_hist is NULL");
    if (!c->kept_tp.m) return fail(ECDNA_E_STATE, std::string("pool_accepted_timepoints") + kNeedsTimepoints);
    if (!c->launched || !c->acc.valid)
        return fail(ECDNA_E_STATE, "pool_accepted_timepoints before accept (a launch invalidates the acceptance results; "
                                   "ecdna_ssa_ctx_create_keep_timepoints)");
    if (threshold >= c->acc.rows)
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
    const std::string bad = ecdna::select::invalid_pass("select_digits", pass, n_prefixes, prefixes, out_hist);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    CheckedSource src;
    TRY(checked_source(c, source, timepoint_mask, "select_digits", kNoQuantile, &src));
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
    const std::string bad = sel::invalid_ranks("select", K, s->ranks, s->fractions);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    if (s->reserved) return fail(ECDNA_E_INVALID, "select.reserved must be 0");
    CheckedSource src;
    TRY(checked_source(c, s->source, s->timepoint_mask, "select", kNoQuantile, &src));
    return sel::run(K, s->ranks, s->fractions, [&](uint32_t pass, const uint64_t* prefixes, uint64_t* hist) {
        return select_pass(c, s->source, src, pass, K, prefixes, sel::kMaxRanks, hist, "ecdna_ssa_ctx_select");
    }, out_population, out_ranks, out_values, out_counts_le);
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
    } else if (!c->sdr.keys_valid || !sd::same(c->sdr.block, *a, c->p.hist_bins)) {
        return fail(ECDNA_E_STATE, "select_draws_digits: pass " + std::to_string(pass) +
                                       " has no keys to read: pass 0 of the same block must come first (a launch "
                                       "drops the keys)");
    }
    return select_draws_pass(c, a->n_draws, pass, n_prefixes, prefixes, n_prefixes, out_hist, who);
}

int ecdna_ssa_ctx_select_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t n_ranks,
                               const uint64_t* ranks, const double* fractions, uint64_t* out_population,
                               uint64_t* out_ranks, double* out_values, uint64_t* out_counts_le) {
    namespace sel = ecdna::select;
    const char* who = "ecdna_ssa_ctx_select_draws";
    if (!c) return fail(ECDNA_E_INVALID, "ctx is NULL");
    const std::string bad = ecdna::select_draws::invalid_ranks(n_ranks, ranks, fractions);
    if (!bad.empty()) return fail(ECDNA_E_INVALID, bad);
    KeptStore* s = nullptr;
    TRY(select_draws_store(c, a, &s));
    const bool any = c->p.n_replicates != 0u;  // (none: every pass counts nothing)
    if (any) {
        TRY(hipSetDevice(c->device));
        TRY(select_draws_keys(c, *s, *a, who));
    }
    return sel::run(n_ranks, ranks, fractions, [&](uint32_t pass, const uint64_t* prefixes, uint64_t* hist) {
        return any ? select_draws_pass(c, a->n_draws, pass, n_ranks, prefixes, sel::kMaxRanks, hist, who) : ECDNA_OK;
    }, out_population, out_ranks, out_values, out_counts_le);
}

}  // extern "C"
