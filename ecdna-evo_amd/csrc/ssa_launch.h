// ssa_launch.h — host-visible kernel argument blocks and launch wrappers shared by the device
// code (steppers: ssa_kernels.hip, ssa_refdraws.hip; end-of-run passes: ssa_hist.hip,
// ssa_subsample.hip, ssa_snapstats.hip, ssa_passage.hip, ssa_cohort.hip; the passes over the kept samples:
// ssa_rescore.hip, ssa_thin.hip, ssa_accept_draws.hip, ssa_pool_draws.hip; the acceptance pass: ssa_accept.hip; the select passes:
// ssa_select.hip) and ssa_api.cpp
// (the C ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ecdna_ssa.h"

namespace ecdna {

// Replicate rotation (bin store): replicates are split into kRotParts partitions, one per XCD (the
// XCC id of the lane's CU), so a parked replicate is only ever resumed by a CU that shares the L2 it
// was parked through. Partition x holds the replicates r with r mod kRotParts == x; its waiting
// replicates are found by walking its items: item j is replicate x + kRotParts * (j % rot_n_pad) (pass
// j / rot_n_pad: round-robin order; slots past the chunk are DONE); rot_n_pad is a multiple of kRotBlock.
constexpr uint32_t kRotParts = 8;
constexpr uint32_t kRotBlock = 16;
constexpr uint32_t kParkVecs = 4;    // 64 B of scalars per parked replicate
enum RotState : uint32_t { ROT_FRESH = 0, ROT_RUNNING = 1, ROT_PARKED = 2, ROT_DONE = 3 };
struct alignas(128) RotPart {
    unsigned long long head;        // items walked
    int waiting;                    // FRESH + PARKED replicates (never below the number of such flags)
    int fresh;                      // FRESH replicates
    uint32_t pad[28];
};

// One chunk of replicates for the persistent SSA stepper.
struct StepperArgs {
    uint16_t* rows;                 // [n][row_stride] per-replicate N+ rows (replicate-major)
    ecdna_rep_summary_t* summaries; // [n], already offset to the chunk
    uint32_t* head;                 // work counter (zeroed before the launch)
    const uint32_t* order;          // [n] chunk-local start order (costliest sets first) or nullptr: id order
    const float4* rates;            // [n_param_sets] (b0, b1, d0, d1)
    const uint16_t* init_copies;
    const uint32_t* init_offsets;   // [n_sets + 1] or nullptr (shared initial distribution)
    const uint64_t* init_nminus_set;// [n_sets] or nullptr
    uint64_t row_stride;            // cells per row (multiple of 64 -> 128-B aligned rows)
    uint64_t seed;
    uint64_t rid0;                  // global id of the chunk's first replicate
    uint64_t rid_stride;            // global-id step between the chunk's replicates (>= 1)
    uint64_t reps_per_set;
    uint64_t max_cells;
    uint64_t stop_cells;            // MaxCells when n- + n+ >= stop_cells: max_cells, or
                                    // ceil(max_cells / 2) under ECDNA_FLAG_BD_CAP_COMPAT (birth-death)
    uint64_t init_nminus;
    double max_time;
    float max_time32;
    uint32_t n;                     // replicates in the chunk
    uint32_t init_nplus;
    uint32_t max_iter;
    uint32_t cell_cap;
    uint32_t flags;
    uint32_t n_snap;                // snapshots (0 = none)
    const uint64_t* snap_cells;     // [n_snap], ascending
    ecdna_snapshot_t* snap_meta;    // [n][n_snap], chunk-offset
    uint16_t* snap_rows;            // [n][n_snap][snap_stride] or nullptr, chunk-offset
    uint64_t snap_stride;           // cells per snapshot row (cell_cap rounded up)
    uint32_t big_cap;               // bin store: large-k row capacity (<= cell_cap, <= row_stride)
    void* bags;                     // bin store: [n][bin_k] final u16 / u32 bin counters (chunk-local)
    // bin store drain control: waves in SIMD wave slots >= admit_slot (the youngest) take no fresh
    // replicate once fewer than admit_remaining are left; admit_slot = 0xffffffff: off
    uint32_t admit_slot;
    uint32_t admit_remaining;
    // bin store replicate rotation ("Rotation"): every 2^rot_tick_log2 loop iterations a
    // wave parks its lanes' replicates (bin counters -> bags, scalars -> park) and its lanes pull the next
    // waiting replicate of their XCD's partition, so all replicates advance together and none starts
    // late. rot_parts = nullptr: off.
    RotPart* rot_parts;             // [kRotParts] (host-initialised per launch)
    uint32_t* rot_flags;            // [kRotParts * rot_n_pad]: RotState per replicate
    uint4* rot_park;                // [n][kParkVecs] parked scalars
    uint32_t rot_n_pad;             // replicates per partition, multiple of kRotBlock
    uint32_t rot_tick_log2;
    int32_t rot_park_min;           // park at a tick only if at least this many replicates wait
    // reference draws (ECDNA_FLAG_REFERENCE_DRAWS, ssa_refdraws.hip): the ChaCha8 key of seed_from_u64(seed)
    // (8 words) and the BTPE constants of Binomial(2k, 1/2) per copy number k (refdraws::kBtpeRow doubles)
    const uint32_t* ref_key;
    const double* ref_btpe;
    uint64_t* rng_words;            // [n] chunk-offset: ChaCha8 words each replicate's stream handed out (or nullptr)
    // serial passaging (ecdna_ssa_passages_t; ssa_passage.hip): a growth phase g > 0 starts replicate i (chunk-local)
    // from the founders the previous phase's sample left, founder_counts[i] = {n-, n+} and the n+ copy numbers
    // founder_rows[i][0 .. n+) in ascending order, instead of the run's initial distribution. nullptr / 0: phase 0 and
    // every other run. Only the instances kFlagPassageRt selects read them: the bin stepper's runtime-flags instances
    // and the row stepper's FND = true instances.
    const uint16_t* founder_rows;   // [n][founder_stride]
    const uint2* founder_counts;    // [n]
    uint64_t founder_stride;        // cells per founder row (passage_cells rounded up to 64)
};

// What the end-of-run passes share, embedded by value in their argument blocks and filled once per chunk and phase.
// The chunk's replicates and how a pass splits them: local replicate r has the global id rid0 + r * rid_stride and
// belongs to parameter set id / reps_per_set; workgroup w walks replicates [w * reps_per_block, ...).
struct ChunkIds {
    uint64_t rid0;
    uint64_t rid_stride;                  // >= 1
    uint64_t reps_per_set;
    uint32_t n;
    uint32_t bins;
    uint32_t reps_per_block;
};
// The target of the ABC distances: its CDF over the bins and its mean / entropy / N+ frequency; has = 0: no distances.
struct StatsTarget {
    const double* cdf;                    // [bins]
    double mean, entropy, freq;
    uint32_t has;
};
// The final state the steppers left: rows and summaries, and in the bin store the per-replicate counters
// [n][bag_k] (u16, or u32 when bag_c32) beside the large-k cells at the head of each row; bags = nullptr: rows only.
struct FinalState {
    const uint16_t* rows;
    const ecdna_rep_summary_t* summaries; // chunk-offset
    uint64_t row_stride;
    const void* bags;
    uint32_t bag_k;
    uint32_t bag_c32;
};
// The BAG template parameter of the passes: 0 = rows only, 1 / 2 = u16 / u32 bin counters.
inline int bag_index(const void* bags, uint32_t bag_c32) { return bags ? (bag_c32 ? 2 : 1) : 0; }
inline int bag_index(const FinalState& fs) { return bag_index(fs.bags, fs.bag_c32); }

// Histogram / totals pass over one chunk. The final state's fields stand here one by one, hist and totals between
// them: ssa_hist<false, 0> and ssa_hist_bags (the passes the bench times) read the first 64 bytes with one scalar
// load, and with FinalState embedded they compiled to other instructions (docs/PERF_LOG.md).
struct HistArgs {
    const uint16_t* rows;                 // FinalState.rows, .summaries
    const ecdna_rep_summary_t* summaries;
    uint64_t* hist;                       // [n_sets][bins]
    unsigned long long* totals;           // [n_sets][16] (ecdna_totals_t as u64 words)
    uint64_t row_stride;                  // FinalState.row_stride
    ChunkIds ids;
    ecdna_rep_stats_t* stats;             // chunk-offset: per-replicate ABC statistics (nullptr = off)
    StatsTarget target;
    const void* bags;                     // FinalState.bags, .bag_k, .bag_c32
    uint32_t bag_k;
    uint32_t bag_c32;
};

// End-of-run subsampling pass over one chunk (ssa_subsample.hip; params.subsample_cells > 0): per replicate, the
// statistics of a sample of m cells of its final state, and the per-set sum of the samples' histograms.
struct SubsampleArgs {
    FinalState state;
    ChunkIds ids;
    StatsTarget target;
    ecdna_rep_stats_t* stats;             // chunk-offset: the samples' statistics
    uint64_t* sample_hist;                // [n_sets][bins]
    uint64_t seed;
    uint32_t m;                           // sample size (cells), 1 .. kMaxSubsampleCells
    uint32_t table_slots;                 // per-wave table of drawn positions: subsample_table_slots(m)
};

// Per-snapshot ABC statistics over one chunk (ssa_snapstats.hip; ecdna_ssa_ext_t.snapshot_stats): for every replicate
// and snapshot, the statistics of the saved state (and of a sample of m of its cells), and per snapshot and set the
// sum of the saved states' (the samples') histograms. A snapshot that was not taken counts as an empty population.
struct SnapStatsArgs {
    ChunkIds ids;
    const ecdna_snapshot_t* snap_meta;    // [n][n_snap], chunk-offset
    const uint16_t* snap_rows;            // [n][n_snap][snap_stride]: the chunk's snapshot rows (expanded u16 rows)
    ecdna_rep_stats_t* stats;             // [n][n_snap], chunk-offset
    ecdna_rep_stats_t* sample_stats;      // [n][n_snap], chunk-offset; nullptr when m == 0
    uint64_t* hist;                       // [n_snap][n_sets][bins]
    uint64_t* sample_hist;                // [n_snap][n_sets][bins]; nullptr when m == 0
    const double* target_cdf;             // [n_snap][bins]: each snapshot's own target, or nullptr (no distances)
    const double* target_scalars;         // [n_snap][3]: the targets' mean, entropy, N+ frequency
    uint64_t snap_stride;
    uint64_t seed;
    uint32_t n_snap;
    uint32_t n_sets;
    uint32_t m;                           // sample size (cells), 0 = no samples, <= kMaxSubsampleCells
    uint32_t table_slots;                 // per-wave table of drawn positions: subsample_table_slots(m), 0 when m == 0
};

// The passage pass over one chunk (ssa_passage.hip; ecdna_ssa_passages_t): per replicate, the sample of m cells of the
// phase's final state by subsample mapping v1 (statistics and per-set histogram exactly as SubsampleArgs' pass), and,
// unless this is the last phase, the sample's cells as the next phase's founders.
struct PassageArgs {
    FinalState state;
    ChunkIds ids;
    StatsTarget target;
    ecdna_rep_stats_t* stats;             // chunk-offset: the samples' statistics
    uint64_t* sample_hist;                // [n_sets][bins]
    uint16_t* founder_rows;               // [n][founder_stride], chunk-local: the sample's N+ copy numbers, ascending;
                                          // nullptr: no founders (the last phase)
    uint2* founder_counts;                // [n], chunk-local: {n-, n+} of the sample
    uint64_t founder_stride;              // >= m
    uint64_t seed;                        // the phase's key seed_g
    uint32_t m;                           // sample size (cells), 1 .. kMaxSubsampleCells
    uint32_t table_slots;                 // per-wave table of drawn positions: subsample_table_slots(m)
    uint32_t sort_slots;                  // per-wave founder array (u16): passage_sort_slots(m)
    // the snapshot keep pass only (launch_keep_snapshots; ecdna_ssa_keep_timepoints_t): one population per (replicate,
    // snapshot) pair of the chunk. state.rows / .row_stride are the chunk's snapshot rows [n][n_snap][row_stride] (no
    // summaries, no counters); founder_rows / founder_counts are slice 0 of the run's kept cells [T][n_run][m] and
    // headers [T][n_run] at the chunk's offset, and snapshot s goes to slice s, slice_stride samples further on.
    const ecdna_snapshot_t* snap_meta;    // [n][n_snap], chunk-offset
    uint64_t slice_stride;                // samples per timepoint slice: the run's replicates
    uint32_t n_snap;
};

// The cohort pass over one chunk (ssa_cohort.hip; ecdna_ssa_cohort_t, cohort mapping v1): per replicate, the statistics
// of its final state against each of P targets, and of its sample of m_p cells against target p. The targets are grouped
// by distinct sample size in order of first appearance (ssa_cohort.hpp): group g draws one sample of group_m[g] cells and
// scores it against the targets group_targets[group_offset[g] .. group_offset[g + 1]). The groups travel in the argument
// block itself: wave-uniform, read with scalar loads. Records lie [P][out_stride].
constexpr uint32_t kMaxCohortTargets = 64;  // P: one bit each of a 64-bit timepoint mask, one lane each of a wave
struct CohortArgs {
    FinalState state;
    ChunkIds ids;
    ecdna_rep_stats_t* stats;             // [P][out_stride], offset to the chunk: the full populations' statistics
    ecdna_rep_stats_t* sample_stats;      // likewise the samples'; nullptr when n_groups == 0
    uint64_t out_stride;                  // records per target: the run's replicates
    const double* target_cdf;             // [P][bins]
    const double* target_scalars;         // [P][3]: the targets' mean, entropy, N+ frequency
    uint64_t seed;
    uint32_t n_targets;                   // P, 1 .. kMaxCohortTargets
    uint32_t n_groups;                    // distinct sample sizes, 0 (no samples) .. P
    uint32_t table_slots;                 // per-wave table of drawn positions: subsample_table_slots(largest m), or 0
    uint32_t scratch_words;               // per-wave u32 words shared by that table and the population's CDF (f64 per
                                          // bin): cohort_scratch_words(bins, table_slots)
    uint32_t group_m[kMaxCohortTargets];
    uint32_t group_offset[kMaxCohortTargets + 1];
    uint32_t group_targets[kMaxCohortTargets];
};

// The kept samples (ecdna_ssa_keep_t, keep mapping v1). The keep pass over one chunk is ssa_passage's KEEP instance on a
// PassageArgs block: founder_rows / founder_counts are the run's kept cells [n][m] and headers [n] at the chunk's offset,
// founder_stride = m; stats, sample_hist and target are not read. The passes over the kept samples of the whole run:
// ssa_rescore scores them against P targets given after the launch, one wave per replicate (records [P][n]);
struct RescoreArgs {
    const uint2* headers;                 // [n] {n-, n+}; {0xffffffff, 0xffffffff}: the guard ended the sample
    const uint16_t* cells;                // [n][m]: the N+ cells' true copy numbers
    ecdna_rep_stats_t* out;               // [P][n]
    const double* target_cdf;             // [P][bins]
    const double* target_scalars;         // [P][3]: the targets' mean, entropy, N+ frequency
    uint32_t n;                           // replicates of the run
    uint32_t m;                           // keep_cells
    uint32_t bins;
    uint32_t n_targets;                   // P, 1 .. kMaxCohortTargets
    uint32_t reps_per_block;
};
// ssa_pool_accepted sums, per global parameter set, the histograms of the kept samples whose mask bit q is set (hist
// zeroed on the stream before it);
struct PoolAcceptedArgs {
    const uint2* headers;
    const uint16_t* cells;
    const uint32_t* mask;                 // [n]: the acceptance pass's
    unsigned long long* hist;             // [n_sets][bins]
    uint64_t rid0, rid_stride, reps_per_set;
    uint32_t n;
    uint32_t m;
    uint32_t bins;
    uint32_t q;                           // the threshold row, < kMaxAcceptRows
    uint32_t reps_per_block;
};
// ssa_kept_gather copies the kept samples of the listed replicates, one wave each, in the list's order.
struct KeptGatherArgs {
    const uint2* headers;
    const uint16_t* cells;
    const uint32_t* index;                // [n_ids]: replicate indices of the call, each < n (checked on the host)
    uint2* out_headers;                   // [n_ids]
    uint16_t* out_cells;                  // [n_ids][m]
    uint32_t n_ids;
    uint32_t m;
};
// ssa_thin (ssa_thin.hip; ecdna_ssa_ctx_rescore_sized, thinning mapping v1) scores one slice of kept samples, each
// target on its own number of measured cells: the kept sample of header {a, b} is the population "a N- cells, then
// cells[0 .. b)", and a target of m1 < a + b cells is scored on the sample of m1 cells that subsample mapping v1 draws
// from it on the slice's thinning stream. The targets are grouped by (m1, draw index) in order of first appearance
// (ssa_thin.hpp): group g draws one sample of group_m[g] cells on stream group_tag[g] — a group whose m1 reaches a + b
// scores the whole kept sample instead, which depends on the replicate — and scores it against the targets
// group_targets[group_offset[g] .. group_offset[g + 1]). Every target is in one group. The groups travel in the argument
// block itself: wave-uniform, read with scalar loads. Records lie [P][n], as RescoreArgs'.
struct ThinArgs {
    const uint2* headers;                 // [n]
    const uint16_t* cells;                // [n][m]
    ecdna_rep_stats_t* out;               // [P][n]
    const double* target_cdf;             // [P][bins]
    const double* target_scalars;         // [P][3]
    uint64_t seed;                        // the key the slice's own samples were drawn under
    uint64_t rid0, rid_stride;            // replicate i of the run has the global id rid0 + i * rid_stride
    uint32_t n;                           // replicates of the run
    uint32_t m;                           // keep_cells
    uint32_t bins;
    uint32_t n_targets;                   // P, 1 .. kMaxCohortTargets
    uint32_t reps_per_block;
    uint32_t n_groups;                    // 1 .. P
    uint32_t table_slots;                 // per-wave table of drawn positions: subsample_table_slots(largest m'), or 0
    uint32_t scratch_words;               // per-wave u32 words shared by that table and the scored sample's CDF:
                                          // cohort_scratch_words(bins, table_slots)
    uint32_t group_m[kMaxCohortTargets];
    uint32_t group_tag[kMaxCohortTargets];  // counter word 1 of the group's draws, without the block index t
    uint32_t group_offset[kMaxCohortTargets + 1];
    uint32_t group_targets[kMaxCohortTargets];
};
constexpr uint32_t kKeptGuard = 0xffffffffu;  // both words of the header of a sample the guard ended
constexpr int kPoolBlock = 256;
constexpr int kGatherBlock = 256;

// The acceptance pass over the whole run (ssa_accept.hip; ecdna_ssa_ctx_accept, acceptance mapping v1): ABC rejection
// over statistics the context already holds. Replicate i's record of timepoint t is stats[i * rep_stride + t * tp_stride]
// (one record: strides 1, 0; snapshots [n][S]: S, 1; passages [G][n]: 1, n) and the error word of its phase t is
// summaries[i + t * err_stride].error (err_stride 0: one summary per replicate, whatever t). The thresholds travel in
// the argument block itself: wave-uniform, read with scalar loads.
constexpr uint32_t kMaxAcceptRows = 32;  // threshold rows Q: one bit each of a replicate's 32-bit mask
constexpr int kAcceptBlock = 256;
struct AcceptArgs {
    const ecdna_rep_stats_t* stats;
    const ecdna_rep_summary_t* summaries;
    uint64_t rep_stride, tp_stride, err_stride;
    uint64_t tmask;                       // participating timepoints (bits below T; never 0 for T > 0)
    uint64_t rid0, rid_stride, reps_per_set;  // replicate i of the run has the global id rid0 + i * rid_stride
    uint32_t n;                           // replicates of the run
    uint32_t T;                           // timepoints of the source
    uint32_t Q;                           // threshold rows, 1 .. kMaxAcceptRows
    uint32_t n_sets;
    uint32_t* mask;                       // [n]: bit q = accepted under row q
    unsigned long long* counts;           // [Q][n_sets], zeroed before the launch
    // the list of the replicates accepted under row list_q, in ascending i (ordered stream compaction)
    uint32_t list_q;
    uint32_t n_blocks;                    // workgroups of kAcceptBlock replicates: ceil(n / kAcceptBlock)
    uint32_t* block_counts;               // [n_blocks]: accepted per workgroup, then (scanned) accepted before it
    uint64_t list_capacity;               // entries ids / list_stats hold
    uint64_t* ids;                        // [list_capacity] global ids
    ecdna_rep_stats_t* list_stats;        // [list_capacity][T]
    double thr[kMaxAcceptRows][4];        // per row: ks, mean_rel, entropy_rel, frequency_diff (+inf: off)
};

// The flat group tables of the passes over thinning draws: slice s of a store owns the groups slice_group[s] ..
// slice_group[s + 1), and group g draws one sample of group_m[g] cells per draw and scores or pools it for the targets
// group_targets[group_offset[g] .. group_offset[g + 1]) (indices into target_cdf / target_scalars), as ThinArgs' groups.
// accept_draws::plan (ssa_accept_draws.hpp) makes them; they travel in the argument block: wave-uniform, read with
// scalar loads.
struct Grouping {
    uint32_t n_groups;                    // over all slices, 1 .. n_targets
    uint32_t slice_group[kMaxCohortTargets + 1];
    uint32_t group_m[kMaxCohortTargets];  // 1 .. m each
    uint32_t group_offset[kMaxCohortTargets + 1];
    uint32_t group_targets[kMaxCohortTargets];
};
// Whether a kernel may index by g's tables on a store of n_slices slices of m kept cells and n_targets targets: every
// index it forms from them stays inside them, target_cdf and a kept row.
inline bool grouping_ok(const Grouping& g, uint32_t n_slices, uint32_t n_targets, uint32_t m) {
    if (n_slices < 1u || n_slices > kMaxCohortTargets || n_targets < 1u || n_targets > kMaxCohortTargets ||
        g.n_groups < 1u || g.n_groups > n_targets || g.slice_group[0] != 0u || g.slice_group[n_slices] != g.n_groups ||
        g.group_offset[0] != 0u || g.group_offset[g.n_groups] > n_targets)
        return false;
    for (uint32_t s = 0; s < n_slices; ++s)
        if (g.slice_group[s] > g.slice_group[s + 1u]) return false;
    for (uint32_t j = 0; j < g.n_groups; ++j)
        if (g.group_offset[j] > g.group_offset[j + 1u] || g.group_m[j] < 1u || g.group_m[j] > m) return false;
    for (uint32_t j = 0; j < g.group_offset[g.n_groups]; ++j)
        if (g.group_targets[j] >= n_targets) return false;
    return true;
}

// What the two passes over thinning draws share (ssa_accept_draws.hip, ssa_pool_draws.hip): the store, the targets and
// the range of draws. The store's slices 0 .. n_slices - 1 (headers [n_slices][n], cells [n_slices][n][m]) are walked
// per replicate; slice s takes part in the verdict when bit s of slice_mask is set and draws under slice_seed[s] on
// stream slice_tag[s] with the draw index set (thin::draw_tag). The keep store is one slice; the timepoint store a slice
// per timepoint. The error words lie as AcceptArgs' (err_stride 0: one summary per replicate; else slice s's is
// summaries[i + s * err_stride], over the slices of slice_mask).
constexpr uint32_t kThinDraws = 64;      // thinning draws of one kept sample: the draw index takes 6 bits
struct DrawsArgs {
    const uint2* headers;                 // [n_slices][n]
    const uint16_t* cells;                // [n_slices][n][m]
    const ecdna_rep_summary_t* summaries;
    const double* target_cdf;             // [targets][bins]
    const double* target_scalars;         // [targets][3]
    uint64_t err_stride;
    uint64_t slice_mask;                  // participating slices (bits below n_slices, never 0)
    uint64_t rid0, rid_stride, reps_per_set;
    uint32_t n;                           // replicates of the run
    uint32_t m;                           // the store's kept cells per sample
    uint32_t bins;
    uint32_t n_slices;                    // 1 .. 64
    uint32_t n_targets;                   // rows of target_cdf, 1 .. kMaxCohortTargets
    uint32_t n_sets;
    uint32_t first_draw, n_draws;         // first_draw + n_draws <= kThinDraws, n_draws >= 1
    uint32_t reps_per_block;
    uint32_t table_slots;                 // as ThinArgs', for the largest m' of any group
    uint32_t scratch_words;
    uint64_t slice_seed[kMaxCohortTargets];
    uint32_t slice_tag[kMaxCohortTargets];  // thin::stream_tag(field, 0)
};

// The thinned acceptance pass over the whole run (ssa_accept_draws.hip; ecdna_ssa_ctx_accept_draws, thinned acceptance
// mapping v1): per replicate and threshold row, the number of thinning draws first_draw .. first_draw + n_draws - 1 on
// which acceptance mapping v1 accepts the records ssa_thin would write for that draw — the records stay in registers.
// The keep store's one slice has the participating targets' groups; a slice of the timepoint store one group of one
// target. Tables and thresholds travel in the argument block: wave-uniform, read with scalar loads (below the 4 KiB a
// launch takes).
struct AcceptDrawsArgs {
    DrawsArgs s;
    Grouping g;
    uint8_t* passes;                      // [n][Q]
    unsigned long long* sums;             // [Q][n_sets], zeroed before the launch
    uint32_t Q;                           // threshold rows, 1 .. kMaxAcceptRows
    double thr[kMaxAcceptRows][4];        // per row: ks, mean_rel, entropy_rel, frequency_diff (+inf: off)
};
static_assert(sizeof(AcceptDrawsArgs) <= 4096, "the argument block of a launch");

// The pooling pass over thinning draws (ssa_pool_draws.hip; ecdna_ssa_ctx_pool_draws, thinned pooling mapping v1): per
// replicate the 64-bit set of the draws it passes under the one threshold row thr — AcceptDrawsArgs' verdict for that
// row, over the groups of `verdict` on the participating slices — and then, for a replicate that passes any, the pools
// over every slice of the store: kept[s] takes popcount(set) times the slice's full histogram, thinned[target] the
// thinned histograms of the passing draws of the target's group in `pool` (the pooling grouping: every slot, whatever
// the mask). Either output may be null: it is then neither computed nor written.
struct PoolDrawsArgs {
    DrawsArgs s;                          // table_slots: for the largest m' of either grouping
    Grouping verdict, pool;
    unsigned long long* thinned;          // [n_targets][n_sets][bins] or null, zeroed before the launch
    unsigned long long* kept;             // [n_slices][n_sets][bins] or null, zeroed before the launch
    uint32_t wave_words;                  // per-wave u32 words of LDS: pool_draws_wave_words(bins, table_slots)
    double thr[4];                        // the row: ks, mean_rel, entropy_rel, frequency_diff (+inf: off)
};
static_assert(sizeof(PoolDrawsArgs) <= 4096, "the argument block of a launch");

// The select passes over the whole run (ssa_select.hip; ecdna_ssa_ctx_select / _select_digits, select mapping v1): an
// 8-bit radix select of order statistics of the four distances. ssa_select_keys writes every replicate's key per
// distance once per (source, timepoint mask), from records and error words that lie as AcceptArgs' do;
// ssa_select_digits counts, per pass, distance and distinct prefix, the keys with that prefix by their next 8 bits.
constexpr uint32_t kMaxSelectGroups = 32;  // distinct prefixes per distance and pass (the ranks K of a call at most)
constexpr int kSelectBlock = 256;
struct SelectKeyArgs {
    const ecdna_rep_stats_t* stats;
    const ecdna_rep_summary_t* summaries;
    uint64_t rep_stride, tp_stride, err_stride;
    uint64_t tmask;                       // participating timepoints (bits below T; never 0 for T > 0)
    uint64_t* keys;                       // [4][n]: per distance the maximum key over the participating timepoints,
                                          // select::kExcluded for a replicate with an error
    uint32_t n;                           // replicates of the run
    uint32_t T;                           // timepoints of the source
};
struct SelectArgs {
    const uint64_t* keys;                 // [4][n]
    unsigned long long* hist;             // [4][kMaxSelectGroups][256], zeroed before the launch
    uint32_t n;
    uint32_t pass;                        // 0 .. 7: the keys' bits 63 - 8 * pass .. 56 - 8 * pass are the digit
    uint32_t reps_per_block;              // consecutive replicates a workgroup walks (>= 1)
    uint32_t n_groups[4];                 // per distance, distinct prefixes: 1 .. kMaxSelectGroups (pass 0: 1)
    uint64_t prefix[4][kMaxSelectGroups]; // their top 8 * pass bits, shifted down (pass 0: 0); wave-uniform reads
};

// The keys of the select over thinning draws (ssa_select_draws.hip; ecdna_ssa_ctx_select_draws, thinned select mapping
// v1): per replicate, draw of the range and distance, the maximum over the participating groups' targets of the key of
// the record AcceptDrawsArgs' pass scores on that draw. Entry i * n_draws + (d - first_draw) of each distance's array;
// ssa_select_digits then walks them as SelectArgs' keys with n = s.n * s.n_draws, which is below 2^32.
struct SelectDrawsArgs {
    DrawsArgs s;
    Grouping g;
    uint64_t* keys;                       // [4][n * n_draws]; select::kExcluded for a replicate with an error
};
static_assert(sizeof(SelectDrawsArgs) <= 4096, "the argument block of a launch");

constexpr uint32_t kMaxSubsampleCells = 4096;  // LDS: 8 B of table per sampled cell and wave (<= 32 KiB)
constexpr int kStepperBlock = 256;
constexpr int kBinWideBlock = 64;  // bin store with 256 bins
constexpr int kHistBlock = 256;
constexpr uint32_t kMaxHistBins = 4096;  // LDS: 8 B per bin per workgroup (<= 64 KiB)
constexpr uint32_t kMaxSnapshots = 64;
// Internal flag bit (never a user flag): the run takes snapshots. With f32 time and the event hash it selects the bin
// stepper's runtime-flags instances (TF = 1); the TF = 0 instances (the bench's) compile snapshots, f32 time and the
// hash out, which frees the scalar registers the snapshot test held across the event loop.
constexpr uint32_t kFlagSnapshotsRt = 0x80000000u;
// Internal flag bit: the run is a passage run (ecdna_ssa_passages_t), set for every phase from phase 0 on. It selects the
// bin stepper's runtime-flags instances too: only they hold the start from founders and its big_cap guard.
constexpr uint32_t kFlagPassageRt = 0x40000000u;
constexpr uint32_t kRuntimeFlagMask =
    ECDNA_FLAG_TIME_F32 | ECDNA_FLAG_EVENT_HASH | kFlagSnapshotsRt | kFlagPassageRt;
constexpr uint32_t kMaxPassages = 16;

// Kernel handle for occupancy queries and the launch itself.
// window: 1 = LDS tail window variant (default), 0 = rows straight in HBM (A/B reference); flags: kFlagPassageRt selects
// the instances whose replicate start reads a passage run's founders (launch_stepper: a.flags)
const void* stepper_kernel(int birth_death, int segregation, int window, uint32_t flags = 0);
hipError_t launch_stepper(const StepperArgs& a, int birth_death, int segregation, int window, uint32_t blocks,
                          hipStream_t stream);
// Bin store (ECDNA_FLAG_BIN_STORE): bin_k = 64 or 256 binned copy numbers; c32 = u32 counters
// (cell_cap > 65535); flags selects the compile-time variant without f32 time and event hash when
// neither is set. bin_stepper_block = the variant's workgroup size.
// ilp: 1 = the max-ILP instruction schedule of the same kernels (a second compile of ssa_kernels.hip,
// ECDNA_ILP_BUILD): fewer stalls for lone waves, more VGPRs (3 waves per SIMD); the ABI takes it when a
// chunk has at most one wave of replicates per SIMD. ilp = 2: for K = 64 / u16, the
// default schedule capped at 128 VGPRs (4 workgroups per CU instead of 3), taken when lanes run many
// replicates each; other K / counter widths fall back to the default schedule.
const void* bin_stepper_kernel(int birth_death, int segregation, uint32_t bin_k, int c32, uint32_t flags, int ilp);
const void* bin_stepper_kernel_ilp(int birth_death, int segregation, uint32_t bin_k, int c32, uint32_t flags);
// ilp = 3: the max-ILP schedule with paired lanes (lane l < 32 owns a replicate, lane l + 32 helps its N-
// fast-forward; birth-death, K = 32 / u32 or K = 64): nullptr where no such instance exists. A paired
// workgroup of kStepperBlock lanes runs kStepperBlock / 2 replicates at a time.
const void* bin_stepper_kernel_pair(int segregation, uint32_t bin_k, int c32, uint32_t flags);
int bin_stepper_block(uint32_t bin_k);
hipError_t launch_bin_stepper(const StepperArgs& a, int birth_death, int segregation, uint32_t bin_k, int c32, int ilp,
                              uint32_t blocks, hipStream_t stream);
hipError_t launch_hist(const HistArgs& a, uint32_t blocks, hipStream_t stream);
// The sampling passes (ssa_subsample.hip, ssa_passage.hip, ssa_snapstats.hip) run one wave per population, each wave
// with its own histogram, table of drawn positions (2 * pow2ceil(m) slots) and, in the passage pass, founder array
// (pow2ceil(m) u16 slots, at least 64) in dynamic LDS. pass_waves: 1, 2 or 4 waves per workgroup, as many as keep
// fixed_bytes + waves * per_wave_bytes (*lds_bytes) within 64 KiB; one wave may exceed it, which the launch refuses.
constexpr size_t kPassLdsMax = 65536;
inline uint32_t pass_waves(size_t fixed_bytes, size_t per_wave_bytes, size_t* lds_bytes) {
    uint32_t nw = 4;
    while (nw > 1u && fixed_bytes + nw * per_wave_bytes > kPassLdsMax) nw >>= 1;
    if (lds_bytes) *lds_bytes = fixed_bytes + nw * per_wave_bytes;
    return nw;
}
inline uint32_t pow2_from(uint32_t p, uint32_t m) {
    while (p < m) p <<= 1;
    return p;
}
inline uint32_t subsample_table_slots(uint32_t m) { return 2u * pow2_from(1u, m); }
inline uint32_t passage_sort_slots(uint32_t m) { return pow2_from(64u, m); }
// ssa_subsample: the workgroup's u64 sum of the samples' histograms; per wave histogram, prefix sums, table (u32)
inline uint32_t subsample_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, size_t* lds_bytes) {
    return pass_waves((size_t)bins * 8u, ((size_t)bins + bag_k + table_slots) * 4u, lds_bytes);
}
// ssa_passage: no workgroup histogram (at the limits, 2,048 bins beside m = 4096, one wave takes 49 KiB); per wave
// histogram, prefix sums, table (u32) and founders (u16)
inline uint32_t passage_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, uint32_t sort_slots,
                              size_t* lds_bytes) {
    return pass_waves(0, ((size_t)bins + bag_k + table_slots + (sort_slots >> 1)) * 4u, lds_bytes);
}
// ssa_snapstats: the workgroup's u64 sum of the saved states' histograms and, if any workgroup size leaves room for
// it (*sample_hist_lds), of the samples' (else the waves add their samples' bins to global memory); per wave
// histogram and table (u32)
inline uint32_t snapstats_waves(uint32_t bins, uint32_t table_slots, size_t* lds_bytes, bool* sample_hist_lds) {
    for (int in_lds = table_slots ? 1 : 0;; --in_lds) {
        size_t lds = 0;
        const uint32_t nw = pass_waves((size_t)bins * (in_lds ? 16u : 8u), ((size_t)bins + table_slots) * 4u, &lds);
        if (lds <= kPassLdsMax || in_lds == 0) {
            if (lds_bytes) *lds_bytes = lds;
            if (sample_hist_lds) *sample_hist_lds = in_lds != 0;
            return nw;
        }
    }
}
// ssa_cohort: no workgroup histogram (the cohort keeps none); per wave the full histogram, the sample's histogram,
// prefix sums, and one scratch area that holds the table (u32) while a sample is drawn and the population's CDF (f64
// per bin) while it is scored (at the limits, 2,048 bins beside m = 4096 and K = 256, one wave takes 49 KiB)
inline uint32_t cohort_scratch_words(uint32_t bins, uint32_t table_slots) {
    return table_slots > 2u * bins ? table_slots : 2u * bins;
}
inline uint32_t cohort_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, size_t* lds_bytes) {
    return pass_waves(0, (2u * (size_t)bins + bag_k + cohort_scratch_words(bins, table_slots)) * 4u, lds_bytes);
}
// the keep pass (ssa_passage's KEEP instance): the passage pass's plan — per wave histogram, prefix sums, table (u32)
// and the kept cells (u16) while they are sorted; no workgroup histogram
inline uint32_t keep_waves(uint32_t bins, uint32_t bag_k, uint32_t table_slots, uint32_t sort_slots,
                           size_t* lds_bytes) {
    return passage_waves(bins, bag_k, table_slots, sort_slots, lds_bytes);
}
// ssa_rescore: per wave the kept sample's histogram (u32 per bin) and its CDF (f64 per bin): 24 KiB at 2,048 bins
inline uint32_t rescore_waves(uint32_t bins, size_t* lds_bytes) {
    return pass_waves(0, (size_t)bins * 4u + (size_t)bins * 8u, lds_bytes);
}
// ssa_thin: per wave the kept sample's full histogram, the thinned sample's histogram, and one scratch area that holds
// the table (u32) while a sample is drawn and the scored sample's CDF (f64 per bin) while it is scored: 8 + 8 + 16 KiB at
// 2,048 bins and keep_cells = 4096 (m' <= 2048: a table of 4,096 slots), two waves per workgroup
inline uint32_t thin_waves(uint32_t bins, uint32_t table_slots, size_t* lds_bytes) {
    return pass_waves(0, (2u * (size_t)bins + cohort_scratch_words(bins, table_slots)) * 4u, lds_bytes);
}
// ssa_pool_draws: ssa_thin's per-wave plan plus the wave's pooled accumulator, [bins] u32 rounded up to an even number
// of words (the next wave's CDF stays 8-byte aligned). The accumulator lives only while samples are drawn and none is
// scored, so it lies in the scratch behind the table, where the CDF's upper part would be, and the plan grows only by
// the words that do not fit there: none when 2 * bins >= table_slots + bins (ssa_thin's plan and occupancy, e.g. 1,025
// bins beside keep_cells = 200), all of them at 2,048 bins and keep_cells = 4096 (8 + 8 + 16 + 8 = 40 KiB, one wave
// per workgroup).
inline uint32_t pool_draws_wave_words(uint32_t bins, uint32_t table_slots) {
    const uint32_t scratch = cohort_scratch_words(bins, table_slots), need = table_slots + bins + (bins & 1u);
    return 2u * bins + (need > scratch ? need : scratch);
}
inline uint32_t pool_draws_waves(uint32_t bins, uint32_t table_slots, size_t* lds_bytes) {
    return pass_waves(0, (size_t)pool_draws_wave_words(bins, table_slots) * 4u, lds_bytes);
}
// Whether a kernel may index its LDS, the store, the targets and its outputs by s (the group tables: grouping_ok): what
// launch_accept_draws and launch_pool_draws refuse of the part they share.
inline bool draws_ok(const DrawsArgs& s) {
    return s.scratch_words == cohort_scratch_words(s.bins, s.table_slots) && s.n_slices >= 1u &&
           s.n_slices <= kMaxCohortTargets && s.n_targets >= 1u && s.n_targets <= kMaxCohortTargets && s.n_draws >= 1u &&
           s.first_draw < kThinDraws && s.n_draws <= kThinDraws - s.first_draw && s.n && s.reps_per_block &&
           s.bins >= 2u && s.rid_stride && s.reps_per_set && s.n_sets && s.m && s.slice_mask &&
           !(s.n_slices < 64u && (s.slice_mask >> s.n_slices)) && s.headers && s.cells && s.summaries && s.target_cdf &&
           s.target_scalars;
}
// ssa_pool_accepted: the workgroup's u64 sum of the accepted samples' histograms (one parameter set at a time), 16 KiB
// at 2,048 bins; its waves keep nothing of their own
inline uint32_t pool_accepted_waves(uint32_t bins, size_t* lds_bytes) {
    if (lds_bytes) *lds_bytes = (size_t)bins * 8u;
    return (uint32_t)kPoolBlock / 64u;
}
// the snapshot keep pass (ssa_passage's KEEP = 2 instance): the keep pass's plan over a population that is a row only
// (bag_k = 0) — per wave histogram, table (u32) and the kept cells (u16) while they are sorted: 8 + 32 + 8 KiB at 2,048
// bins and m = 4096, one wave per workgroup
inline uint32_t keep_snapshots_waves(uint32_t bins, uint32_t table_slots, uint32_t sort_slots, size_t* lds_bytes) {
    return passage_waves(bins, 0u, table_slots, sort_slots, lds_bytes);
}
hipError_t launch_keep(const PassageArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_keep_snapshots(const PassageArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_rescore(const RescoreArgs& a, hipStream_t stream);
hipError_t launch_thin(const ThinArgs& a, hipStream_t stream);
hipError_t launch_pool_accepted(const PoolAcceptedArgs& a, hipStream_t stream);
hipError_t launch_kept_gather(const KeptGatherArgs& a, hipStream_t stream);
hipError_t launch_subsample(const SubsampleArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_cohort(const CohortArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_snapstats(const SnapStatsArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_passage(const PassageArgs& a, uint32_t blocks, hipStream_t stream);
// The acceptance pass (ssa_accept.hip): every replicate's mask and the per-set counts (a.counts zeroed on the stream
// before it), and — launch_accept_list, after it on the same stream — the ordered list of the replicates accepted under
// row a.list_q: per-workgroup counts, their exclusive scan by one workgroup, the scatter. Three launches, no workgroup
// ever waits for another. a.n > 0.
hipError_t launch_accept_mask(const AcceptArgs& a, hipStream_t stream);
hipError_t launch_accept_list(const AcceptArgs& a, hipStream_t stream);
// The thinned acceptance pass (ssa_accept_draws.hip): ssa_thin's LDS plan (thin_waves) for a.s.table_slots; a.sums zeroed
// on the stream before it. A block that disagrees with the plan is refused: hipErrorInvalidValue.
hipError_t launch_accept_draws(const AcceptDrawsArgs& a, hipStream_t stream);
// The pooling pass over thinning draws (ssa_pool_draws.hip): pool_draws_waves' LDS plan for a.s.table_slots; a.thinned
// and a.kept zeroed on the stream before it. A block that disagrees with the plan is refused: hipErrorInvalidValue.
hipError_t launch_pool_draws(const PoolDrawsArgs& a, hipStream_t stream);
// The keys of the select over thinning draws (ssa_select_draws.hip): ssa_thin's LDS plan (thin_waves) for
// a.s.table_slots. A block that disagrees with the plan, or whose keys 32 bits do not index, is refused:
// hipErrorInvalidValue.
hipError_t launch_select_draws_keys(const SelectDrawsArgs& a, hipStream_t stream);
// The select passes (ssa_select.hip): the keys of every replicate (a.n > 0), and one digit pass over them (a.hist zeroed
// on the stream before it; the dynamic LDS table is 1 KiB per group of the distance with most, 32 KiB at most).
hipError_t launch_select_keys(const SelectKeyArgs& a, hipStream_t stream);
hipError_t launch_select_digits(const SelectArgs& a, hipStream_t stream);
// The reference-draws stepper (row store; ssa_refdraws.hip)
const void* refdraws_kernel(int birth_death, int segregation);
int refdraws_block();
hipError_t launch_refdraws(const StepperArgs& a, int birth_death, int segregation, uint32_t blocks,
                           hipStream_t stream);

}  // namespace ecdna
