/*
 * ecdna_ssa.h — C ABI of the MI355X many-replicate Gillespie SSA engine for
 * ecDNA birth–death–segregation dynamics.
 *
 * This is the drop-in boundary for the reference's hot path. In
 * fraterenz/ecdna-evo v0.26.0 every replicate is one call of
 *
 *     sosa::simulate(&mut state, &rates, &reactions, &mut process, &options, &mut rng)
 *
 * (src/main.rs:92-99 for PureBirth, src/main.rs:166-173 for BirthDeath), made
 * once per replicate index idx by the closure run_simulations
 * (src/main.rs:55-211) that rayon maps over seed*10 .. seed*10+runs
 * (src/main.rs:212-225). Inside that call run the process model
 * (AdvanceStep::advance_step / update_state, src/process.rs:114-197 and
 * src/process.rs:259-345), the event kernels (Exponential::increase_nplus,
 * increase_nminus, CellDeath::decrease_nplus / decrease_nminus,
 * src/proliferation.rs:24-140) and the segregation rules
 * (src/segregation.rs:110-194).
 *
 * Here ONE call runs ALL replicates of a run on one GPU (one replicate per
 * GPU lane): ecdna_ssa_run() replaces the R calls of simulate() that the
 * rayon loop makes, and returns what run_simulations keeps of each one
 * (stop reason, final [n-, n+] and time: src/main.rs:124-128, 198-210) plus
 * the pooled copy-number histogram that process::save writes per replicate
 * (src/process.rs:31-55; JSON body {"0": n-, "k": cells}, dynamics.md:8).
 *
 * Conventions: plain C types only; no exceptions cross the boundary; every
 * buffer is caller-owned; functions return 0 on success or a negative
 * ECDNA_E_* code (ecdna_ssa_strerror). Per-replicate failures that the
 * reference turns into panics are reported in ecdna_rep_summary_t.error.
 *
 * RNG: replicate r (a GLOBAL id, so shards on different GPUs draw the same
 * streams as one big run) uses Philox4x32-10 with key = (seed lo, seed hi)
 * and counter = (event index, sub-block, r lo, r hi). The draw mapping is
 * spelled out in DESIGN.md §3; oracle/ restates it on the CPU bit for bit.
 */
#ifndef ECDNA_SSA_H
#define ECDNA_SSA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Added within v13 (additive: no layout and no existing function changes, the version stays 13): ABC thresholds over
 * thinning draws — ecdna_ssa_ctx_select_draws and its shard primitive ecdna_ssa_ctx_select_draws_digits (below; thinned
 * select mapping v1): exact order statistics of the four distances over the pairs (replicate, thinning draw) of a block
 * ecdna_ssa_accept_draws_t without threshold rows, found by the radix select of ecdna_ssa_ctx_select over keys that no
 * stored record stands behind. A context that never calls them allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): the accepted
 * thinnings pooled — ecdna_ssa_ctx_pool_draws (below; thinned pooling mapping v1): per global parameter set, the
 * histograms of the thinned samples on the draws that pass one threshold row of ecdna_ssa_accept_draws_t, and the whole
 * kept samples weighted by the number of passing draws, in one synchronous pass. A context that never calls it allocates
 * and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): acceptance over
 * repeated thinnings of the kept samples — the block ecdna_ssa_accept_draws_t, ecdna_ssa_ctx_accept_draws and
 * ecdna_ssa_ctx_download_accept_draws (below; thinned acceptance mapping v1): per replicate and threshold row, on how many
 * of up to 64 thinning draws the replicate is accepted, counted in one pass that stores no record. A context that never
 * calls them allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): the kept samples
 * rescored at each target's own number of measured cells — the block ecdna_ssa_rescore_t, ecdna_ssa_ctx_rescore_sized
 * and ecdna_ssa_ctx_rescore_timepoints_sized (below; thinning mapping v1). They write the records of
 * ecdna_ssa_ctx_rescore and _rescore_timepoints; a context that never calls them allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): the sample of every
 * timepoint of a longitudinal run kept on the GPU — the timepoint keep block ecdna_ssa_keep_timepoints_t and
 * ecdna_ssa_ctx_create_keep_timepoints, late scoring of a longitudinal target (ecdna_ssa_ctx_rescore_timepoints,
 * ecdna_ssa_ctx_download_rescored_timepoints and the acceptance source ECDNA_ACCEPT_RESCORED_TIMEPOINTS), the posterior
 * predictive histogram per timepoint ecdna_ssa_ctx_pool_accepted_timepoints and the kept cells themselves,
 * ecdna_ssa_ctx_download_kept_timepoints (below; timepoint keep mapping v1). ecdna_ssa_ctx_create_keep(p, ext, passages,
 * cohort, keep, out) is ecdna_ssa_ctx_create_keep_timepoints(p, ext, passages, cohort, keep, NULL, out): a context
 * without the block allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): every replicate's
 * sample kept on the GPU, scored and pooled after the sweep — the keep block ecdna_ssa_keep_t and
 * ecdna_ssa_ctx_create_keep, late scoring against targets that were not known at create (ecdna_ssa_ctx_rescore,
 * ecdna_ssa_ctx_download_rescored and the acceptance source ECDNA_ACCEPT_RESCORED), the posterior predictive histogram
 * ecdna_ssa_ctx_pool_accepted and the kept cells themselves, ecdna_ssa_ctx_download_kept (below; keep mapping v1).
 * ecdna_ssa_ctx_create_cohort(p, ext, passages, cohort, out) is ecdna_ssa_ctx_create_keep(p, ext, passages, cohort, NULL,
 * out): a context without the block allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): one sweep scored
 * against a cohort of targets on the GPU — several patients, or several biopsies of one tumour, each with its own
 * copy-number histogram and its own number of measured cells: the cohort block ecdna_ssa_cohort_t,
 * ecdna_ssa_ctx_create_cohort and ecdna_ssa_ctx_download_cohort, and the acceptance sources ECDNA_ACCEPT_COHORT and
 * ECDNA_ACCEPT_COHORT_SAMPLES (below; cohort mapping v1). ecdna_ssa_ctx_create_passages(p, ext, passages, out) is
 * ecdna_ssa_ctx_create_cohort(p, ext, passages, NULL, out): a context without the block allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): ABC thresholds on the
 * GPU — exact order statistics of the distances among the error-free replicates by an 8-bit radix select over the
 * statistics a context already holds, ecdna_ssa_ctx_select and its shard primitive ecdna_ssa_ctx_select_digits (below;
 * select mapping v1). A context that never calls them allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): ABC rejection on the
 * GPU — the acceptance pass ecdna_ssa_ctx_accept / ecdna_ssa_ctx_download_accept over the statistics a context already
 * holds (below; acceptance mapping v1). A context that never calls it allocates and launches nothing new.
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): serial passaging —
 * every replicate regrown from its own sample on the GPU, the reference's cell-line strategy: the passage block
 * ecdna_ssa_passages_t, ecdna_ssa_ctx_create_passages and ecdna_ssa_ctx_download_passages (below; passage mapping v1).
 * ecdna_ssa_ctx_create_ext(p, ext, out) is ecdna_ssa_ctx_create_passages(p, ext, NULL, out).
 * Added within v13 (additive: no layout and no existing function changes, the version stays 13): per-snapshot ABC
 * statistics on the GPU for longitudinal inference — the extension block ecdna_ssa_ext_t, ecdna_ssa_ctx_create_ext and
 * ecdna_ssa_ctx_download_snapshot_stats (below). ecdna_ssa_ctx_create(p, out) is ecdna_ssa_ctx_create_ext(p, NULL, out).
 * ABI v13: end-of-run subsampling on the GPU. ecdna_ssa_params_t gains subsample_cells and reserved1 (appended after
 * reserved0, so the v10-v12 layout is a prefix of this one) and ecdna_ssa_ctx_download_sample returns the statistics
 * and the per-set histogram of a sample of subsample_cells cells of every replicate's final population (subsample
 * mapping v1, below). With subsample_cells = 0 no new kernel is launched and every output is v12's; the draw mapping
 * is v8 as before.
 * ABI v12: draw mapping v8, the time step as the soft log times the correctly rounded reciprocal RN32(1 / a0) (v7
 * divided: the correctly rounded quotient; the two differ by at most one ulp, so results differ from v11's for the
 * same seed). The Params layout and everything else are those of v11.
 * ABI v11: ECDNA_REP_ERR_INTERNAL (a replicate whose event would pick from an empty N+ set stops instead of
 * indexing off its row); unknown flag bits are rejected; the lane-quad schedule (instance schedule 4) is gone.
 * The Params layout is that of v10 (v10 appended ecdna_ssa_params_t.max_workgroups, a cap on the persistent grid for
 * contexts that share a GPU; v9 took the channel from all 32 bits of the event's word over f64 cumulative
 * propensities, draw mapping v7). */
#define ECDNA_SSA_ABI_VERSION 13

/* Process type — ProcessType (src/clap_app.rs:311-315); chosen as BirthDeath
 * when d0 > 0 or d1 > 0 (src/clap_app.rs:163-174, 194-200). */
typedef enum {
    ECDNA_PURE_BIRTH = 0,  /* channels [ProliferateNMinus, ProliferateNPlus]  src/main.rs:67-71 */
    ECDNA_BIRTH_DEATH = 1  /* + [DeathNMinus, DeathNPlus]                     src/main.rs:139-145 */
} ecdna_process_t;

/* Segregation rule — SegregationOptions (src/clap_app.rs:232-238). */
typedef enum {
    ECDNA_SEG_DETERMINISTIC = 0,      /* Deterministic      src/segregation.rs:142-155 */
    ECDNA_SEG_BINOMIAL = 1,           /* Binomial           src/segregation.rs:110-140 */
    ECDNA_SEG_BINOMIAL_NO_UNEVEN = 2, /* BinomialNoUneven   src/segregation.rs:157-174 */
    ECDNA_SEG_BINOMIAL_NO_NMINUS = 3  /* BinomialNoNminus   src/segregation.rs:176-194 */
} ecdna_seg_t;

/* Reaction channels, in the reference's channel order (src/main.rs:140-145).
 * EcDNAEvent (src/process.rs:20-29) declares 7 variants; only these 4 are
 * reachable (src/process.rs:179, 331). */
typedef enum {
    ECDNA_EV_PROLIF_NMINUS = 0,
    ECDNA_EV_PROLIF_NPLUS = 1,
    ECDNA_EV_DEATH_NMINUS = 2,
    ECDNA_EV_DEATH_NPLUS = 3
} ecdna_event_t;

/* Why a replicate stopped (sosa::StopReason; checked in this order before
 * every event). */
typedef enum {
    ECDNA_STOP_NONE = 0,       /* never started (see error) */
    ECDNA_STOP_MAX_CELLS = 1,  /* n- + n+ >= max_cells        (Options.max_cells, src/clap_app.rs:207) */
    ECDNA_STOP_MAX_TIME = 2,   /* t >= max_time               (IterTime.time, src/clap_app.rs:205) */
    ECDNA_STOP_MAX_ITER = 3,   /* iterations >= max_iter      (MAX_ITER, src/main.rs:23) */
    ECDNA_STOP_ABSORBING = 4,  /* total propensity == 0 (extinction) */
    ECDNA_STOP_ERROR = 5       /* see ecdna_rep_summary_t.error */
} ecdna_stop_t;

/* Per-replicate errors — where the reference panics or refuses. */
typedef enum {
    ECDNA_REP_OK = 0,
    ECDNA_REP_ERR_OVERFLOW = 1,   /* 2k > u16::MAX: checked_mul panic, src/proliferation.rs:63-67 */
    ECDNA_REP_ERR_EMPTY = 2,      /* empty initial distribution: ensure!, src/process.rs:88, 232 */
    ECDNA_REP_ERR_CELL_CAP = 3,   /* N+ row would exceed cell_cap (the reference grows a Vec), or the
                                     bin store's large-k row would exceed big_cap */
    ECDNA_REP_ERR_REJECTION = 4,  /* BinomialNoUneven loop exceeded 4096 redraws (p < 2^-4096) */
    ECDNA_REP_ERR_INTERNAL = 5    /* an N+ event drawn with no N+ cell, or a cell index past n+ (ABI v11): the event
                                     is not applied and the replicate stops. Unreachable under draw mapping v8 (a
                                     zero-propensity channel is never drawn); the guard keeps a broken invariant
                                     from indexing off the row. The reference's pick_remove_random_nplus returns an
                                     error on an empty N+ set (src/proliferation.rs:57). */
} ecdna_rep_error_t;

/* Flags (ecdna_ssa_params_t.flags). */
#define ECDNA_FLAG_TIME_F32 0x1u       /* accumulate time in f32 like process.time (src/process.rs:68, 184) */
#define ECDNA_FLAG_BD_CAP_COMPAT 0x2u  /* BD: stop at 2(n- + n+) >= max_cells, i.e. sum of the
                                          duplicated population vector (src/process.rs:339-344) */
#define ECDNA_FLAG_EVENT_HASH 0x4u     /* fold every event into ecdna_rep_summary_t.event_hash */
#define ECDNA_FLAG_SNAPSHOT_ROWS 0x8u  /* keep the N+ row of every snapshot (else only its metadata) */
#define ECDNA_FLAG_REP_STATS 0x10u     /* per-replicate ABC statistics (ecdna_rep_stats_t) */
/* Cell store of a replicate's N+ cells. Default: the ROW store, one u16 per cell
 * in the reference's swap_remove order (ecdna-lib EcDNADistribution.nplus: Vec<u16>). With this flag:
 * the BIN store, per-replicate counts of cells by copy number k = 1..bin_kmax held in LDS, plus a
 * row of the cells with k > bin_kmax. A uniform cell pick has the same law under any arrangement
 * of the cells, so both stores simulate the same process; they consume the same draws but address
 * cells in a different order, so their runs differ seed for seed (each is bit-exact with its own
 * oracle restatement). Final and snapshot rows come back in canonical order: k = 1 cells, k = 2
 * cells, ..., k = bin_kmax cells, then the large-k row. */
#define ECDNA_FLAG_BIN_STORE 0x20u
/* Reference draw structure (row store only; not with ECDNA_FLAG_BIN_STORE): instead of the engine's Philox
 * mapping, replicate r draws exactly what the Rust reference draws for replicate index r — ChaCha8Rng
 * seed_from_u64(seed) on stream seed*10 + r (src/main.rs:56-58), the first-reaction method over f32
 * propensities with rand_distr's Exp1 ziggurat, gen_range + swap_remove for cell picks, rand_distr's
 * Binomial (BINV / BTPE) for segregation — and accumulates time in f32 (process.time, src/process.rs:184;
 * ECDNA_FLAG_TIME_F32 is implied). log and exp are the correctly rounded functions (the reference's glibc
 * calls agree with them wherever glibc rounds correctly). A correctness path for seed-for-seed comparison
 * with the reference semantics, not a fast path. */
#define ECDNA_FLAG_REFERENCE_DRAWS 0x40u
/* Every defined flag; ecdna_ssa_ctx_create rejects other bits (ABI v11). */
#define ECDNA_FLAG_ALL 0x7fu

/* API return codes. */
#define ECDNA_OK 0
#define ECDNA_E_INVALID (-1)   /* bad parameter */
#define ECDNA_E_HIP (-2)       /* HIP runtime error */
#define ECDNA_E_NOMEM (-3)     /* device allocation failed */
#define ECDNA_E_NODEVICE (-4)  /* no usable gfx950 device */
#define ECDNA_E_STATE (-5)     /* call order (e.g. download before launch) */
#define ECDNA_E_COMM (-6)      /* RCCL error, or librccl.so.1 not loadable (multi-GPU reduction only) */

/* Rates of one parameter set: ReactionRates([b0, b1, d0, d1]) (src/main.rs:67, 139). f32 as in Cli
 * (src/clap_app.rs:41-55). Each must be 0 or in [2^-60, 2^60] (else ECDNA_E_INVALID; the reference does not
 * check them; since ABI v8): the f32 propensities (rate x population, u32 populations) and the f32 total a0 of
 * the time step then stay normal and finite, which the stepper's time-step division relies on. */
typedef struct {
    float b0, b1, d0, d1;
} ecdna_rates_t;

/* One run = n_replicates independent replicates; replicate i of the call (i = 0 .. n_replicates - 1)
 * has global id r = first_replicate + i * replicate_stride (stride 0 or 1: the contiguous ids
 * first_replicate .. first_replicate + n_replicates - 1). Replicate r uses parameter set
 * s = r / reps_per_set (must be < n_param_sets). Every draw is keyed by r, so a replicate's results do
 * not depend on which call, device or position runs it: G calls with first_replicate = g and
 * replicate_stride = G (g = 0 .. G-1) together run the same replicates as one call, interleaved so
 * that every call gets the same mix of parameter sets (balanced ABC sweeps across GPUs). */
typedef struct {
    int32_t process;                /* ecdna_process_t */
    int32_t segregation;            /* ecdna_seg_t */
    const ecdna_rates_t* rates;     /* host, [n_param_sets] */
    uint32_t n_param_sets;          /* 1, or e.g. 1024 for an ABC sweep */
    uint32_t hist_bins;             /* bins per set: bin 0 = N- cells, bin k = cells with k copies,
                                       bin hist_bins-1 = cells with >= hist_bins-1 copies; >= 2 */
    uint64_t reps_per_set;          /* replicates per parameter set (>= 1) */
    uint64_t seed;                  /* --seed (src/clap_app.rs:63) */
    uint64_t first_replicate;       /* global id of the first replicate of this call (sharding) */
    uint64_t n_replicates;          /* replicates in this call */
    uint64_t max_cells;             /* stop when n- + n+ >= max_cells (src/clap_app.rs:142-157). Populations are
                                       u32: a max_cells above 2^32 - 1 acts as 2^32 - 1 */
    double max_time;                /* stop when t >= max_time (years; src/clap_app.rs:151, 205) */
    uint64_t max_iter;              /* stop after max_iter events (1e9, src/main.rs:23); < 2^32 */
    uint32_t cell_cap;              /* capacity of the per-replicate N+ row (cells); rounded up to 64 */
    uint32_t flags;                 /* ECDNA_FLAG_* */
    /* Initial distribution (EcDNADistribution: n- plus one u16 per N+ cell; default {1: 1},
     * src/clap_app.rs:188-191). Either shared by every set (init_set_offsets == NULL: copies
     * init_copies[0 .. init_nplus), n- = init_nminus) or per set (init_set_offsets[n_param_sets+1]
     * into init_copies, init_set_nminus[n_param_sets]). Copy numbers must be >= 1, and every set's initial
     * n- + n+ must be < 2^32 (ECDNA_E_INVALID otherwise): cell counts are u32 in every stepper. A final state of
     * 2^32 - 1 cells is reachable (it stops at once with MaxCells); its sample is the guard's (subsample mapping v1). */
    const uint16_t* init_copies;    /* host */
    uint32_t init_nplus;
    uint32_t bin_kmax;              /* ECDNA_FLAG_BIN_STORE: copy numbers 1..bin_kmax are binned; 32, 64 or
                                       256 (0 = 64); part of the draw mapping (the canonical cell order) */
    uint64_t init_nminus;
    const uint32_t* init_set_offsets; /* host or NULL */
    const uint64_t* init_set_nminus;  /* host or NULL */
    int32_t device;                 /* HIP device ordinal for ecdna_ssa_run / ctx_create */
    uint32_t big_cap;               /* ECDNA_FLAG_BIN_STORE: capacity (cells) of a replicate's large-k row,
                                       the cells with k > bin_kmax; 0 = cell_cap. A division that would put
                                       more cells there stops the replicate with ECDNA_REP_ERR_CELL_CAP. The
                                       device row memory is sized by it, outputs by cell_cap. */
    /* Snapshots (--snapshots, src/clap_app.rs:92-97, 102-134; SavingOptions, src/lib.rs:21-25): cell
     * counts, sorted ascending, at most 64. Before every event, while any REMAINING snapshot equals
     * n- + n+, the FRONT one is popped and the current state saved (src/process.rs:122-145, the
     * reference's pop_front-on-any-match rule). NULL / 0 = none. */
    const uint64_t* snapshot_cells; /* host */
    uint32_t n_snapshots;
    uint32_t replicate_stride;      /* global-id step between consecutive replicates of the call (0 = 1) */
    /* Per-replicate ABC summary statistics (abc.md:38-55; ECDNA_FLAG_REP_STATS): compared against this
     * target copy-number histogram of hist_bins entries (bin 0 = N- cells, last bin = overflow), e.g.
     * the patient's data. NULL: statistics are computed, distances to the target are not. */
    const uint64_t* stats_target_hist; /* host */
    /* Scheduling hint (optional, host, n_param_sets entries): the relative cost of one replicate of each
     * parameter set. Replicates of costlier sets are started first (longest-processing-time order, ties
     * in id order), which shortens the tail of a run whose sets differ in cost, such as an ABC sweep.
     * Results do not depend on it. NULL: replicates start in id order. */
    const float* set_cost_hint;
    /* Persistent-grid cap (since ABI v10): at most this many workgroups (0 = as many as the kernel's occupancy
     * fits on the device). Two contexts launched on two streams of one GPU share its CUs only when their grids
     * leave room for each other, e.g. a shard split by initial copy number onto two bin-store instances
     * (DESIGN.md §7). Results do not depend on it. */
    uint32_t max_workgroups;
    uint32_t reserved0;             /* must be 0 */
    /* End-of-run subsampling (since ABI v13; the reference's into_subsampled(nb, &mut rng), src/main.rs:110-123,
     * 184-197; abc.md:38-55 carries both `cells` and `tumour_cells`): 0 = off; m > 0: after the run, a uniform
     * sample of m cells is drawn from every replicate's final population on the GPU and its statistics and
     * histogram are kept for ecdna_ssa_ctx_download_sample. Needs ECDNA_FLAG_REP_STATS (so hist_bins <= 2048);
     * m <= 4096.
     *
     * Subsample mapping v1. A replicate's final population has N = n- + n+ cells at positions 0 .. N-1 in download
     * order: first the n- N- cells (k = 0), then the N+ cells in the order ecdna_ssa_ctx_download returns its row
     * (row store: row order; bin store: k = 1 .. bin_kmax ascending from the counters, then the large-k row).
     *  - m >= N: the sample is the whole population; its statistics equal ecdna_ssa_ctx_download_stats'.
     *  - m < N: with m' = min(m, N - m), draws u_0, u_1, ... are generated until m' distinct values have appeared;
     *    draw i is new iff it equals no earlier draw, and the picked set is the values of the new draws up to and
     *    including the m'-th new one (the first m' distinct values of an iid uniform sequence: a uniform m'-subset).
     *    If m' = m the picked positions are the sample; otherwise they are the cells left out (sample histogram =
     *    full histogram - picked histogram, likewise the sum of k).
     *  - Draw i is a Lemire draw below N: Philox4x32-10 under the run's key (seed lo, seed hi) on counter
     *    (i, 0xC0000000 | t, r lo, r hi), t = 0, 1, ... (the stepper's sub-blocks are small numbers and
     *    ecdna_host_subsample's are 0x80000000 | block with fewer than 2^30 blocks: disjoint streams). The block's
     *    four words are tried in order: word x gives p = x * N and is accepted as p >> 32 when
     *    (p & 0xffffffff) >= (2^32 - N) mod N; if all four are rejected, block t + 1 follows. r is the GLOBAL
     *    replicate id, so a replicate's sample does not depend on chunk, shard, grid or device.
     *  - Guard: a replicate that has not found m' distinct values within 2^16 draws gets all-zero sample statistics
     *    and adds nothing to the sample histogram (unreachable: m' <= N / 2, so every draw is new with probability
     *    >= 1/2). So does one with N >= 2^32 - 1 and m < N (positions are 32-bit).
     *  - The sample's mean uses every cell's true copy number, not the clipped bin, as the full statistics do. Error
     *    and extinct replicates are treated as the full statistics treat them (N = 0: cells 0, ks 1.0 with a target).
     * This is a different sample from ecdna_host_subsample's for the same seed (Floyd's sequential set does not map
     * onto a wave); both are uniform. */
    uint32_t subsample_cells;
    uint32_t reserved1;             /* must be 0 */
} ecdna_ssa_params_t;

/* Per-replicate summary statistics of the final distribution (cells = n- + n+, copy number k per cell,
 * k = 0 for N- cells; bins as in the histogram). Distances are against params.stats_target_hist. */
typedef struct {
    double mean;           /* sum k / cells                                           */
    double entropy;        /* -sum_k p_k ln p_k, p_k = cells with k copies / cells     */
    double frequency;      /* n+ / cells                                              */
    double ks;             /* max_k |F(k) - F_target(k)|, F = cumulative p over bins  */
    double mean_rel;       /* |mean - mean_t| / mean_t      (|mean - mean_t| if mean_t == 0) */
    double entropy_rel;    /* |entropy - entropy_t| / entropy_t (likewise)            */
    double frequency_diff; /* |frequency - frequency_t|                               */
    uint64_t cells;
} ecdna_rep_stats_t;

/* One saved snapshot of one replicate (what process::save writes, src/process.rs:31-55). */
typedef struct {
    double time;                    /* process.time at the save (before the event's waiting time) */
    uint64_t nminus;
    uint64_t nplus;
    uint32_t taken;                 /* 1 if this snapshot was popped (saved) during the run */
    uint32_t reserved;
} ecdna_snapshot_t;

/* What run_simulations keeps of one replicate (src/main.rs:124-128, 198-210), plus counters. */
typedef struct {
    uint64_t nminus;                /* final n-  (population[0]) */
    uint64_t nplus;                 /* final n+  (population[1]) */
    uint64_t iters;                 /* events executed = advance_step calls */
    uint64_t events_by_type[4];     /* per ecdna_event_t */
    uint64_t uneven;                /* ProliferateNPlus events with a complete uneven split */
    double time;                    /* final process.time (years) */
    uint64_t event_hash;            /* FNV-1a fold of (event, k1, cell index) per event, if enabled */
    uint32_t stop_reason;           /* ecdna_stop_t */
    uint32_t error;                 /* ecdna_rep_error_t */
} ecdna_rep_summary_t;

/* Per-parameter-set sums over the replicates of a call. */
typedef struct {
    uint64_t replicates;
    uint64_t events;                /* sum of iters — the numerator of events/s */
    uint64_t events_by_type[4];
    uint64_t uneven;
    uint64_t nminus;                /* sum of final n- */
    uint64_t nplus;                 /* sum of final n+ */
    uint64_t stop_reasons[6];       /* per ecdna_stop_t */
    uint64_t errors;                /* replicates with error != 0 */
} ecdna_totals_t;

int ecdna_ssa_abi_version(void);
const char* ecdna_ssa_strerror(int code);
/* Detail of the last failure on the calling thread ("" if none). */
const char* ecdna_ssa_last_error_message(void);

/* Number of usable gfx950 devices (0 when none). */
int ecdna_ssa_device_count(void);

/* One-shot: runs every replicate of *p on device p->device and copies the results to HOST buffers
 * (each may be NULL): out_summaries[n_replicates] (replicate first_replicate + i * stride at index i),
 * out_hist[n_param_sets * hist_bins] (zeroed, then filled), out_totals[n_param_sets].
 * stream: a hipStream_t, or NULL for the default (null) stream. Blocks until done. */
int ecdna_ssa_run(const ecdna_ssa_params_t* p, ecdna_rep_summary_t* out_summaries,
                  uint64_t* out_hist, ecdna_totals_t* out_totals, void* stream);

/* Device-resident context for repeated runs (benchmarks, multi-GPU). Inputs are uploaded once at
 * create; rows/summaries/histogram stay in HBM between launches. */
typedef struct ecdna_ssa_ctx ecdna_ssa_ctx;

int ecdna_ssa_ctx_create(const ecdna_ssa_params_t* p, ecdna_ssa_ctx** out);

/* Extension block of ecdna_ssa_ctx_create_ext (added within ABI v13; ecdna_ssa_params_t does not grow).
 *
 * Per-snapshot ABC statistics (abc.md's `timepoint` column: a patient, or a culture, is sampled several times as the
 * tumour grows, and a run is scored against the data of every timepoint). With snapshot_stats = 1, after every chunk's
 * stepper and histogram pass the GPU computes, for every replicate and every snapshot of params.snapshot_cells, the
 * ecdna_rep_stats_t of the saved state (n- N- cells and the snapshot's N+ row), with the definitions of the end-of-run
 * statistics: mean from the true copy numbers, bins clipped at hist_bins - 1, distances against snapshot s's OWN target
 * snapshot_target_hists[s]. A snapshot that was not taken (ecdna_snapshot_t.taken == 0: the replicate never had that
 * many cells before an event) is scored as an empty population — cells, mean, entropy and frequency 0, ks 1.0 with a
 * target — and adds nothing to a histogram; ecdna_ssa_ctx_download_snapshots tells the two cases apart. Needs
 * params.n_snapshots > 0 and ECDNA_FLAG_REP_STATS.
 *
 * Without ECDNA_FLAG_SNAPSHOT_ROWS the snapshot rows are scratch of one chunk (chunk_replicates x n_snapshots rows
 * instead of n_replicates x n_snapshots: large runs chunk instead of failing) and are not downloadable; with it the
 * whole run's rows are kept as before.
 *
 * Sampling at the snapshots: snapshot_subsample_cells = m > 0 also draws a uniform sample of m cells of every taken
 * snapshot by subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above) — the population is the nminus N- cells
 * followed by the snapshot row — and keeps the sample's statistics and histogram. The one difference is the stream:
 * draw i of snapshot s (s = 0 .. n_snapshots - 1 < 64) uses Philox counter
 * (i, 0xC0000000 | (s + 1) << 16 | t, r lo, r hi) with t < 1024, disjoint from the end-of-run sample's (field 0) and
 * from every other snapshot's, so the samples of different timepoints are independent. */
typedef struct {
    uint32_t struct_size;               /* sizeof(ecdna_ssa_ext_t); anything else: ECDNA_E_INVALID */
    uint32_t snapshot_stats;            /* 0 / 1 */
    const uint64_t* snapshot_target_hists; /* host, [n_snapshots][hist_bins], or NULL: no distances */
    uint32_t snapshot_subsample_cells;  /* 0 = off, <= 4096 */
    uint32_t reserved;                  /* must be 0 */
} ecdna_ssa_ext_t;
/* ecdna_ssa_ctx_create with an extension block. ext == NULL or ext->snapshot_stats == 0: nothing more is allocated or
 * launched and every output is ecdna_ssa_ctx_create's (struct_size, reserved and the sample size's range are checked
 * whenever ext is given). */
int ecdna_ssa_ctx_create_ext(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext, ecdna_ssa_ctx** out);

/* Serial passaging (added within ABI v13; the reference's cell-line strategy of longitudinal inference: growth
 * restarts from the subsample — a culture is grown, a few hundred cells are taken and measured, and those same cells
 * found the next flask. The patient strategy, growth continuing from the whole population, is the per-snapshot
 * statistics above). Every replicate is regrown on the GPU from its own sample; nothing but the results leaves the
 * device, so chunked sweeps are covered.
 *
 * Passage mapping v1. A run with n_passages = G and passage_cells = m runs G growth phases g = 0 .. G-1 per replicate
 * r (r the GLOBAL id).
 *  - Key. Phase g runs under Philox key seed_g: seed_0 = seed; for g >= 1, with all arithmetic mod 2^64 (the
 *    splitmix64 finaliser of seed + g * golden ratio),
 *        z = seed + g * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *        z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  seed_g = z ^ (z >> 31).
 *    It is computed on the host: the stepper and the sample pass of phase g receive seed_g where they receive seed in
 *    an ordinary run.
 *  - One phase is an ordinary run: the event index starts at 0 and the time at 0, the spare-word stack is empty, the
 *    hash is at its offset, and the stop checks are those of DESIGN.md §3.1 with the run's max_cells / max_time /
 *    max_iter.
 *  - Phase 0 starts from the run's initial distribution: bit for bit the plain run of the same parameters, and its
 *    sample is the plain run's subsample_cells = m sample.
 *  - End of phase g: the population is sampled by subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above),
 *    unchanged — counter (i, 0xC0000000 | t, r lo, r hi), stream field 0 — under key seed_g. The population is the
 *    one that pass sees in an ordinary run (the replicate's final n- and N+ cells, whatever its stop reason; an
 *    extinct or never-started replicate is N = 0). The sample's statistics and histogram are phase g's measurement.
 *  - Founders of phase g + 1: n- = the number of N- cells in the sample; the N+ cells are the sample's cells with
 *    their TRUE copy numbers (not the clipped bins), in ascending copy-number order — the order an initial histogram
 *    gives (copy numbers ascending), so a phase is replayed by an ordinary run whose initial distribution is the
 *    founders' histogram.
 *  - m >= N carries the whole population. An empty sample founds a phase that stops with ECDNA_REP_ERR_EMPTY after
 *    zero events, exactly like an empty initial distribution; so does a sample the guard ended (2^16 draws, or a
 *    position the state cannot account for).
 *  - Bin store: a replicate with more founders of k > bin_kmax than big_cap stops at its start, after zero events,
 *    with ECDNA_REP_ERR_CELL_CAP; it is reported with no cells (n- = n+ = 0: the founders could not be held), so its
 *    next phase stops with ECDNA_REP_ERR_EMPTY. (A defence: the founders are a subset of a population that never held
 *    more than big_cap such cells, so no run reaches it; it keeps a broken invariant from writing off the row.)
 * Results depend only on (seed, r, parameters): chunks, shards, grids, schedules and rotation reproduce each other
 * bit for bit, as everywhere else. */
typedef struct {
    uint32_t struct_size;                  /* sizeof(ecdna_ssa_passages_t); anything else: ECDNA_E_INVALID */
    uint32_t n_passages;                   /* G, 1 .. 16 */
    uint32_t passage_cells;                /* m, 1 .. 4096, <= cell_cap */
    uint32_t reserved;                     /* must be 0 */
    const uint64_t* passage_target_hists;  /* host, [G][hist_bins]: phase g's own target; NULL:
                                              params.stats_target_hist for all */
} ecdna_ssa_passages_t;
/* ecdna_ssa_ctx_create_ext with a passage block. passages == NULL: ecdna_ssa_ctx_create_ext. Otherwise the run needs
 * ECDNA_FLAG_REP_STATS, and these are rejected (ECDNA_E_INVALID, before a device is touched, the message names the
 * field): params.subsample_cells != 0 (the block owns the sample size), params.n_snapshots != 0, ext->snapshot_stats,
 * ECDNA_FLAG_REFERENCE_DRAWS (continuing a ChaCha8 stream across phases is a different feature), an all-zero target
 * row, out-of-range fields.
 * After a launch, ecdna_ssa_ctx_download, _download_stats, _download_sample and ecdna_ssa_ctx_reduce return the LAST
 * phase's results (rows included where the run is one chunk); ecdna_ssa_ctx_sync returns times summed over the
 * phases (hist_ms includes the passage pass). */
int ecdna_ssa_ctx_create_passages(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                  const ecdna_ssa_passages_t* passages, ecdna_ssa_ctx** out);
/* Every phase's results of the last launch of a passage context (else ECDNA_E_STATE, as before a launch). Any buffer
 * may be NULL. With G = n_passages, n = n_replicates: out_summaries [G][n], out_totals [G][n_param_sets], out_stats
 * [G][n] (the whole final population of the phase), out_sample_stats [G][n] (its sample, cells = the sample's size),
 * out_hist and out_sample_hist [G][n_param_sets][hist_bins]. Distances are against phase g's target. Chunked runs are
 * covered. ecdna_ssa_ctx_reduce reduces the last phase's histogram and totals only: callers sum the shards' per-phase
 * arrays themselves. */
int ecdna_ssa_ctx_download_passages(ecdna_ssa_ctx* c, ecdna_rep_summary_t* out_summaries, ecdna_totals_t* out_totals,
                                    ecdna_rep_stats_t* out_stats, ecdna_rep_stats_t* out_sample_stats,
                                    uint64_t* out_hist, uint64_t* out_sample_hist);

/* A cohort of targets (added within ABI v13): several patients, or several biopsies of one tumour, each with its own
 * copy-number histogram and its own number of measured cells, scored against ONE sweep. The simulations are the
 * expensive part of an ABC inference and do not depend on the target: with the block, one more end-of-run pass per chunk
 * scores every replicate's final state against all P targets, so one sweep serves P inferences. The records stay on the
 * device for ecdna_ssa_ctx_accept / ecdna_ssa_ctx_select (the sources ECDNA_ACCEPT_COHORT and
 * ECDNA_ACCEPT_COHORT_SAMPLES below, where timepoint p is target p), so chunked sweeps are covered.
 *
 * Cohort mapping v1. With P = n_targets, n = n_replicates:
 *  - Full records. stats[p][i] is the ecdna_rep_stats_t of replicate i's whole final population, scored against target
 *    p: byte for byte the record ecdna_ssa_ctx_download_stats returns for the same run with stats_target_hist =
 *    target_hists[p]. mean, entropy, frequency and cells are therefore the same for every p.
 *  - Sample records (sample_cells != NULL). sample_stats[p][i] is byte for byte the record ecdna_ssa_ctx_download_sample
 *    returns for the same run with stats_target_hist = target_hists[p] and subsample_cells = sample_cells[p]. It follows
 *    subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above) unchanged: stream field 0, counter
 *    (i, 0xC0000000 | t, r lo, r hi), the run's key, r the GLOBAL id. Two targets with equal sample_cells see the same
 *    sample. The records do not depend on chunk, shard, grid or device.
 *  - params.stats_target_hist and params.subsample_cells keep their meaning: ecdna_ssa_ctx_download_stats and
 *    ecdna_ssa_ctx_download_sample are unchanged and independent of the block, as is every other output.
 *  - The cohort adds no pooled histograms: the pooled histogram does not depend on a target.
 *  - Buffers are sized by the run — [P][n] records of 64 B, twice when samples are on — and allocated at create:
 *    ECDNA_E_NOMEM if they do not fit (the message says how many bytes were asked for). Chunked runs are covered.
 * Rejected at create (ECDNA_E_INVALID, before a device is touched, the message names the field): a wrong struct_size,
 * n_targets outside 1 .. 64, NULL target_hists, an all-zero target row, a sample_cells[p] outside 1 .. 4096,
 * reserved != 0, ECDNA_FLAG_REP_STATS missing, and a non-NULL passages, or ext->snapshot_stats, together with a cohort
 * block (cohorts of longitudinal targets are a different feature). */
typedef struct {
    uint32_t struct_size;            /* sizeof(ecdna_ssa_cohort_t); anything else: ECDNA_E_INVALID */
    uint32_t n_targets;              /* P, 1 .. 64 (one bit each of a timepoint mask) */
    const uint64_t* target_hists;    /* host, [P][hist_bins], binned as stats_target_hist */
    const uint32_t* sample_cells;    /* host, [P], each 1 .. 4096: target p's sample size m_p; NULL: no samples */
    uint64_t reserved;               /* must be 0 */
} ecdna_ssa_cohort_t;
/* ecdna_ssa_ctx_create_passages with a cohort block. cohort == NULL: exactly ecdna_ssa_ctx_create_passages — nothing
 * more is allocated or launched. The three older create calls forward to this one. */
int ecdna_ssa_ctx_create_cohort(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                const ecdna_ssa_passages_t* passages, const ecdna_ssa_cohort_t* cohort,
                                ecdna_ssa_ctx** out);
/* The cohort records of the last launch, [P][n] each (cohort mapping v1); either buffer may be NULL. ECDNA_E_STATE:
 * before a launch, on a context without the block, and when out_sample_stats is asked for with sample_cells == NULL. */
int ecdna_ssa_ctx_download_cohort(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats /* [P][n] */,
                                  ecdna_rep_stats_t* out_sample_stats /* [P][n] */);

/* Every replicate's sample kept on the GPU (added within ABI v13). The cohort block scores targets that are known at
 * create; with the keep block the sample itself stays on the device after the sweep, so that a target that arrives later
 * (another patient or biopsy, a re-binned or corrected histogram) is scored without a new sweep (ecdna_ssa_ctx_rescore),
 * the copy-number distribution of the accepted simulations — the posterior predictive check — is pooled where the
 * samples lie (ecdna_ssa_ctx_pool_accepted), and the accepted simulations' cells can be fetched
 * (ecdna_ssa_ctx_download_kept). After each chunk's histogram pass, and after its subsample and cohort passes, one more
 * pass writes the chunk's kept samples into run-sized buffers: [n][keep_cells] u16 plus [n] headers, n × m × 2 bytes.
 *
 * Keep mapping v1. With m = keep_cells:
 *  - Replicate i's kept sample is the sample that subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above) defines
 *    for m on its end-of-run population, unchanged: stream field 0, counter (i, 0xC0000000 | t, r lo, r hi), the run's
 *    key, r the GLOBAL id. It is therefore the same sample that subsample_cells = m, and a cohort target with
 *    sample_cells[p] = m, see.
 *  - The header ecdna_kept_t holds the sample's N- and N+ cell counts: nminus + nplus = min(m, N).
 *  - cells[i][0 .. nplus) holds the N+ cells' TRUE copy numbers (not the clipped bins), ascending: the founder format of
 *    passage mapping v1. Entries past nplus are unspecified.
 *  - An extinct or never-started replicate keeps the empty sample {0, 0}.
 *  - A sample the guard ended keeps {0xffffffff, 0xffffffff}: it is rescored as the all-zero record, which is what the
 *    sampling passes write for it, and adds nothing to a pooled histogram.
 *  - A kept sample does not depend on chunk, shard, grid or device. Chunked runs are covered.
 *  - ext, cohort, params.subsample_cells and params.stats_target_hist keep their meaning and stay independent of the
 *    block, as does every other output.
 * Rejected at create (ECDNA_E_INVALID, before a device is touched, the message names the field): a wrong struct_size,
 * keep_cells outside 1 .. 4096, reserved != 0, ECDNA_FLAG_REP_STATS missing, and a non-NULL passages (kept samples of
 * every phase are a different feature). ECDNA_E_NOMEM at create if the [n][m] u16 cells plus the [n] headers do not fit
 * (the message says how many bytes were asked for). */
typedef struct {
    uint32_t struct_size;   /* sizeof(ecdna_ssa_keep_t); anything else: ECDNA_E_INVALID */
    uint32_t keep_cells;    /* m, 1 .. 4096 */
    uint64_t reserved;      /* must be 0 */
} ecdna_ssa_keep_t;
typedef struct { uint32_t nminus, nplus; } ecdna_kept_t;   /* one kept sample's header */
/* ecdna_ssa_ctx_create_cohort with a keep block. keep == NULL: exactly ecdna_ssa_ctx_create_cohort — nothing more is
 * allocated or launched. The four older create calls forward to this one. */
int ecdna_ssa_ctx_create_keep(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                              const ecdna_ssa_passages_t* passages, const ecdna_ssa_cohort_t* cohort,
                              const ecdna_ssa_keep_t* keep, ecdna_ssa_ctx** out);
/* Late scoring: the kept samples of the last launch against n_targets = P targets given now, binned as
 * stats_target_hist. Enqueued on the stream of the last launch, asynchronous, like ecdna_ssa_ctx_accept. Record [p][i] is
 * byte for byte the record ecdna_ssa_ctx_download_sample returns for the same run with stats_target_hist =
 * target_hists[p] and subsample_cells = keep_cells. A later rescore replaces the records (P may differ between calls) and
 * drops the keys ecdna_ssa_ctx_select cached, as a relaunch does; a relaunch invalidates the records. The buffer belongs
 * to the context: allocated at the first call, grown by later ones, freed at destroy.
 * The records are the acceptance source ECDNA_ACCEPT_RESCORED: T = the P of the last rescore, timepoint p is target p,
 * the error rule is the one-summary rule of ECDNA_ACCEPT_FINAL, the records lie [P][n] (rep stride 1, timepoint stride n,
 * error stride 0). ecdna_ssa_ctx_accept, _select and _select_digits take it; before a rescore (and on a context without
 * the block) they return ECDNA_E_STATE.
 * ECDNA_E_INVALID: NULL c, n_targets outside 1 .. 64, NULL target_hists, an all-zero target row. ECDNA_E_STATE: before a
 * launch; a context without the keep block. ECDNA_E_NOMEM leaves the context usable. */
int ecdna_ssa_ctx_rescore(ecdna_ssa_ctx* c, uint32_t n_targets, const uint64_t* target_hists /* host [P][hist_bins] */);
/* The records of the last ecdna_ssa_ctx_rescore, [P][n] (ECDNA_E_STATE before one, and after a relaunch until the next).
 * Synchronises, as the other downloads do. */
int ecdna_ssa_ctx_download_rescored(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out /* [P][n] */);
/* The posterior predictive histogram. Synchronous. For row `threshold` of the last ecdna_ssa_ctx_accept, whatever its
 * source, out_hist[s] is the sum, over the replicates of global parameter set s whose mask bit is set, of their kept
 * samples' histograms, binned as out_hist of ecdna_ssa_ctx_download: bin 0 holds the N- cells, true copy numbers are
 * clipped at hist_bins - 1. The sums are integers: shards' arrays sum to the whole run's.
 * ECDNA_E_STATE: a context without the keep block; no valid accept results (before an accept, after a relaunch).
 * ECDNA_E_INVALID: NULL c, threshold >= Q of that accept, NULL out_hist. */
int ecdna_ssa_ctx_pool_accepted(ecdna_ssa_ctx* c, uint32_t threshold,
                                uint64_t* out_hist /* host [n_param_sets][hist_bins] */);
/* The kept samples of the replicates with the global ids ids[0 .. n_ids) (ids == NULL: the call's first n_ids
 * replicates), gathered on the device in the order of ids, then copied once: it takes ecdna_ssa_ctx_download_accept's
 * out_ids as they come. Either output may be NULL.
 * ECDNA_E_INVALID: NULL c; an id that is not a replicate of this call ((id - first_replicate) is not a multiple of the
 * stride, or its index is >= n_replicates); n_ids above n_replicates when ids is NULL. ECDNA_E_STATE: before a launch; a
 * context without the keep block. */
int ecdna_ssa_ctx_download_kept(ecdna_ssa_ctx* c, uint64_t n_ids,
                                const uint64_t* ids /* host, global ids; NULL: the call's first n_ids replicates */,
                                ecdna_kept_t* out_headers /* [n_ids] */, uint16_t* out_cells /* [n_ids][keep_cells] */);

/* Every timepoint's sample kept on the GPU (added within ABI v13). The keep block above stops at the end of the run. The
 * two longitudinal modes — the snapshots of the patient strategy (ecdna_ssa_ext_t.snapshot_stats) and the growth phases
 * of the cell-line strategy (ecdna_ssa_passages_t) — are where a sweep costs most, and their samples were discarded: a
 * second patient, a re-binned target, the posterior predictive per timepoint or the accepted simulations' cells at each
 * timepoint needed a new sweep. With the timepoint keep block the sample of every (replicate, timepoint) pair stays on
 * the device, in run-sized buffers headers[T][n] and cells[T][n][m] allocated at create: T × n × (2m + 8) bytes. (By
 * arithmetic, not a measurement: 6.7 GB of cells and 0.13 GB of headers for 2^22 replicates at T = 4 and m = 200.)
 * ECDNA_E_NOMEM at create, with the
 * byte count in the message, if they do not fit.
 *
 * Timepoint keep mapping v1. T is the number of timepoints of the context, m = keep_cells. Replicate ids are global.
 *  - A snapshot context (params.n_snapshots = S > 0 and ext->snapshot_stats = 1; T = S): the kept sample of (replicate
 *    r, snapshot s) is the sample that snapshot_subsample_cells = m defines for that pair, unchanged: its population is
 *    "nminus N- cells, then the snapshot row", drawn by subsample mapping v1 on stream field (s + 1) << 16 under the
 *    run's key. ext->snapshot_subsample_cells keeps its meaning and stays independent of the block. A snapshot that was
 *    not taken keeps {0, 0}. The row is never read past min(nplus, the row's stride). The pass runs per chunk after the
 *    snapshot statistics, while the chunk's snapshot rows exist: with or without ECDNA_FLAG_SNAPSHOT_ROWS.
 *  - A passage context (T = G = n_passages): keep_cells must equal passage_cells — the kept sample of phase g is the
 *    sample that founds phase g + 1, and another size on the same stream would be a different sample. The kept sample of
 *    (r, g) is phase g's sample under seed_g, stream field 0 (passage mapping v1). For g < G - 1 its header and cells
 *    are the founders of phase g + 1. The last phase is kept too. A phase that never started (an ECDNA_REP_ERR_EMPTY
 *    phase is one) keeps {0, 0}.
 *  - Both: the format is keep mapping v1's — the header ecdna_kept_t {nminus, nplus} with nminus + nplus = min(m, N),
 *    then the nplus TRUE copy numbers, ascending; {0xffffffff, 0xffffffff} for a sample the guard ended. Nothing depends
 *    on chunk, shard, grid or device. Chunked runs are covered. Every other output of the run is unchanged.
 * Rejected at create (ECDNA_E_INVALID, before a device is touched, the message names the field): a wrong struct_size,
 * reserved != 0, keep_cells outside 1 .. 4096, ECDNA_FLAG_REP_STATS missing, a context with neither a passage block nor
 * ext->snapshot_stats, and a passage block with keep_cells != passage_cells. The end-of-run keep block beside a
 * snapshot context stays legal and independent. */
typedef struct {
    uint32_t struct_size;   /* sizeof(ecdna_ssa_keep_timepoints_t); anything else: ECDNA_E_INVALID */
    uint32_t keep_cells;    /* m, 1 .. 4096 */
    uint64_t reserved;      /* must be 0 */
} ecdna_ssa_keep_timepoints_t;
/* ecdna_ssa_ctx_create_keep with a timepoint keep block. keep_timepoints == NULL: exactly ecdna_ssa_ctx_create_keep —
 * nothing more is allocated or launched, and ecdna_ssa_ctx_instance is unchanged. The five older create calls forward
 * to this one. */
int ecdna_ssa_ctx_create_keep_timepoints(const ecdna_ssa_params_t* p, const ecdna_ssa_ext_t* ext,
                                         const ecdna_ssa_passages_t* passages, const ecdna_ssa_cohort_t* cohort,
                                         const ecdna_ssa_keep_t* keep,
                                         const ecdna_ssa_keep_timepoints_t* keep_timepoints, ecdna_ssa_ctx** out);
/* The four calls over the kept timepoint samples return ECDNA_E_STATE before a launch and on a context without the
 * block (the message names ecdna_ssa_ctx_create_keep_timepoints).
 *
 * Late scoring of one longitudinal target: timepoint t's kept samples against target_hists[t], binned as
 * stats_target_hist. Called again for the next patient. Enqueued on the stream of the last launch, asynchronous. The
 * records lie [T][n]. Record [t][i] is byte for byte: on a passage context, ecdna_ssa_ctx_download_passages'
 * out_sample_stats[t][i] of the same run created with passage_target_hists = target_hists; on a snapshot context,
 * ecdna_ssa_ctx_download_snapshot_stats' out_sample_stats[i][t] of the same run created with snapshot_target_hists =
 * target_hists and snapshot_subsample_cells = m. The records and their validity are the call's own, apart from
 * ecdna_ssa_ctx_rescore's. A later call replaces them and drops the keys ecdna_ssa_ctx_select cached, as
 * ecdna_ssa_ctx_rescore does; a relaunch invalidates them.
 * The records are the acceptance source ECDNA_ACCEPT_RESCORED_TIMEPOINTS = 13: T as above, rep stride 1, timepoint
 * stride n. On a passage context the error rule and strides are ECDNA_ACCEPT_PASSAGE_SAMPLES' (per-phase summaries,
 * every participating phase error-free); on a snapshot context the one-summary rule of ECDNA_ACCEPT_FINAL.
 * ecdna_ssa_ctx_accept, _select and _select_digits take it; before a rescore_timepoints they return ECDNA_E_STATE.
 * ECDNA_E_INVALID: NULL c, NULL target_hists, an all-zero target row (target_hists[t] is named). ECDNA_E_NOMEM leaves the
 * context usable. */
int ecdna_ssa_ctx_rescore_timepoints(ecdna_ssa_ctx* c, const uint64_t* target_hists /* host [T][hist_bins] */);
/* The records of the last ecdna_ssa_ctx_rescore_timepoints, [T][n] (ECDNA_E_STATE before one, and after a relaunch until
 * the next). Synchronises. */
int ecdna_ssa_ctx_download_rescored_timepoints(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out /* [T][n] */);
/* The posterior predictive histogram per timepoint. Synchronous. For row `threshold` of the last ecdna_ssa_ctx_accept,
 * whatever its source and timepoint mask, out_hist[t][s] is the sum, over the accepted replicates of global parameter
 * set s, of their timepoint-t kept samples' histograms. Binning and guard handling are ecdna_ssa_ctx_pool_accepted's. The
 * sums are integers: shards' arrays sum to the whole run's.
 * ECDNA_E_STATE also without valid accept results. ECDNA_E_INVALID: NULL c, threshold >= Q of that accept, NULL out_hist. */
int ecdna_ssa_ctx_pool_accepted_timepoints(ecdna_ssa_ctx* c, uint32_t threshold,
                                           uint64_t* out_hist /* host [T][n_param_sets][hist_bins] */);
/* The kept timepoint samples of the replicates with the global ids ids[0 .. n_ids) (ids == NULL: the call's first n_ids
 * replicates), in the order of ids, every timepoint. The id rules and errors are ecdna_ssa_ctx_download_kept's. Either
 * output may be NULL. */
int ecdna_ssa_ctx_download_kept_timepoints(ecdna_ssa_ctx* c, uint64_t n_ids,
                                           const uint64_t* ids /* host, global ids; NULL: the first n_ids replicates */,
                                           ecdna_kept_t* out_headers /* [T][n_ids] */,
                                           uint16_t* out_cells /* [T][n_ids][keep_cells] */);

/* The kept samples rescored at each target's own number of measured cells (added within ABI v13). A cohort target has
 * its own number of measured cells (ecdna_ssa_cohort_t.sample_cells), and that number is part of the distance's noise;
 * ecdna_ssa_ctx_rescore and _rescore_timepoints score a late target on all keep_cells cells of the kept sample. The two
 * calls below score target p on sample_cells[p] <= keep_cells cells instead, without a new sweep: a patient with 80
 * measured cells against a sweep kept at 200, the hundred measured cells of a flask passaged at thousands
 * (keep_cells == passage_cells stays the bottleneck), the biopsies of one patient with their own cell counts. A uniform
 * m1-subset of a uniform m-subset of a population is a uniform m1-subset of that population (m1 <= min(m, N)), so
 * thinning the kept sample has exactly the law of having measured m1 cells.
 *
 * Thinning mapping v1. The scored object is the kept sample of (replicate r, slice tau): the one slice of the keep
 * block, or timepoint t of the timepoint keep block, with header {a, b} and cells[0 .. b), ascending true copy numbers.
 *  - A header {0xffffffff, 0xffffffff} gives the all-zero record for every target, as ecdna_ssa_ctx_rescore does.
 *  - The population is N_k = a + b cells in this order: positions 0 .. a - 1 are N- cells (k = 0), position a + j is
 *    cells[j]. This is the shape of a snapshot's population ("nminus N- cells, then the row").
 *  - A target with m1 >= N_k is scored on the whole kept sample: its record is byte for byte ecdna_ssa_ctx_rescore's
 *    (respectively _rescore_timepoints') against the same histogram. This covers {0, 0} and populations that were
 *    smaller than m1.
 *  - Otherwise subsample mapping v1 (ecdna_ssa_params_t.subsample_cells above) is applied unchanged to this population
 *    with N = N_k and m = m1: m' = min(m1, N_k - m1) positions, the first m' distinct draws, the complement when
 *    m' != m1, the Lemire draw with rejection, the guard after 2^16 draws (the all-zero record) — under the key and on
 *    the stream below.
 *  - The key is the one under which slice tau's own sample was drawn: the run's seed, or seed_g for growth phase g of a
 *    passage context (passage mapping v1).
 *  - The stream: counter word 1 is base_tau | 0x20000000 | (d << 10) | t, t < 2^10 the block index. base_tau is the tag
 *    slice tau's own sample used — 0xC0000000 for the end of the run and for passage phases, 0xC0000000 | (s + 1) << 16
 *    for snapshot s — and d in 0 .. 63 is the target's draw index: up to 64 independent thinnings of the same kept
 *    sample, which estimate a replicate's acceptance probability under measurement noise. Counter word 0 is the draw
 *    index i, words 2 and 3 the GLOBAL replicate id. t takes bits 0-9, d bits 10-15, the snapshot field bits 16-22, the
 *    thinning flag bit 29, the tag bits 30-31: the fields do not meet. No existing stream has bits 29, 30 and 31 all
 *    set: the steppers use small numbers, ecdna_host_subsample uses 0x80000000 | block with block < 2^30, and the
 *    sampling passes keep bit 29 clear.
 *  - The record is the statistics of the thinned sample — its clipped histogram, its true sum of k, its size m1 and its
 *    N+ count — against the target, computed as the cohort pass scores a group's sample.
 *  - Targets with equal (m1, d) see the same thinned sample.
 *  - Nothing depends on chunk, shard, grid or device.
 *  - A thinned record is NOT byte for byte a relaunch with subsample_cells = m1: the kept cells are sorted and the draw
 *    order is gone. It has the same law.
 *  - ecdna_ssa_ctx_pool_accepted*, ecdna_ssa_ctx_download_kept* still pool and return the whole kept samples.
 *
 * The two calls write the records that ecdna_ssa_ctx_rescore and _rescore_timepoints write: the same buffers [P][n] and
 * [T][n], the same validity rules, the acceptance sources 12 and 13, the same drop of the keys ecdna_ssa_ctx_select
 * cached; ecdna_ssa_ctx_download_rescored*, _accept, _select and _select_digits take them unchanged. With sample_cells
 * == NULL the draws are ignored (a non-zero draw with nothing thinned is legal and has no effect) and the result is
 * byte for byte the unsized call's.
 * ECDNA_E_INVALID (the message names the entry): NULL arguments, a wrong struct_size, reserved != 0, n_targets outside
 * 1 .. 64, an all-zero target row, a draw above 63, sample_cells[p] outside 1 .. keep_cells — a target with more
 * measured cells than were kept cannot be served honestly. ECDNA_E_STATE: before a launch; a context without the block. */
typedef struct {
    uint32_t struct_size;          /* sizeof(ecdna_ssa_rescore_t) */
    uint32_t n_targets;            /* P, 1 .. 64 */
    const uint64_t* target_hists;  /* host [P][hist_bins], no all-zero row */
    const uint32_t* sample_cells;  /* host [P] or NULL (every target: the whole kept sample); each 1 .. keep_cells */
    const uint32_t* sample_draws;  /* host [P] or NULL (all 0); each 0 .. 63 */
    uint64_t reserved;             /* must be 0 */
} ecdna_ssa_rescore_t;
int ecdna_ssa_ctx_rescore_sized(ecdna_ssa_ctx* c, const ecdna_ssa_rescore_t* r);
int ecdna_ssa_ctx_rescore_timepoints_sized(ecdna_ssa_ctx* c, const uint64_t* target_hists /* [T][hist_bins] */,
                                           const uint32_t* sample_cells /* [T] or NULL */, uint32_t draw /* 0..63 */);
/* Use caller-owned DEVICE buffers for the histogram [n_param_sets*hist_bins] u64 and totals
 * [n_param_sets] (e.g. tensors later all-reduced over RCCL). NULL keeps the internal buffer. */
int ecdna_ssa_ctx_set_outputs(ecdna_ssa_ctx* c, uint64_t* d_hist, ecdna_totals_t* d_totals);
/* Enqueue one full run on `stream` (a hipStream_t; NULL = the default stream): zero hist/totals, SSA
 * kernel over all replicates (in memory-bounded chunks), histogram kernel. Asynchronous. */
int ecdna_ssa_ctx_launch(ecdna_ssa_ctx* c, void* stream);
/* Block until the last launch finished; returns its device time in ms (HIP events on the launch
 * stream): ssa_ms = SSA stepper kernels only, hist_ms = histogram/summary kernels (and the
 * subsampling pass when params.subsample_cells > 0, and the snapshot statistics pass under
 * ecdna_ssa_ext_t.snapshot_stats, and the cohort pass under ecdna_ssa_cohort_t, and the keep passes of
 * ecdna_ssa_keep_t and ecdna_ssa_keep_timepoints_t). Either may be NULL. */
int ecdna_ssa_ctx_sync(ecdna_ssa_ctx* c, float* ssa_ms, float* hist_ms);
/* Device pointers of the current outputs. */
int ecdna_ssa_ctx_device_outputs(ecdna_ssa_ctx* c, uint64_t** d_hist, ecdna_totals_t** d_totals);
/* Copy results of the last launch to HOST buffers (each may be NULL). out_rows, if given, receives
 * [n_replicates][row_stride] u16 where row i holds the final N+ copies of replicate i in the
 * engine's swap_remove order (row store) or in canonical order (bin store, ECDNA_FLAG_BIN_STORE);
 * entries past summaries[i].nplus are unspecified. Valid only when the
 * whole run fit in one chunk (ecdna_ssa_ctx_row_stride returns > 0). */
int ecdna_ssa_ctx_download(ecdna_ssa_ctx* c, ecdna_rep_summary_t* out_summaries, uint64_t* out_hist,
                           ecdna_totals_t* out_totals, uint16_t* out_rows);
/* Snapshots of the last launch: meta[n_replicates][n_snapshots] and, under ECDNA_FLAG_SNAPSHOT_ROWS,
 * rows[n_replicates][n_snapshots][row_stride] u16 (the N+ cells at the save, in the order of
 * ecdna_ssa_ctx_download; without the flag rows must be NULL, else ECDNA_E_STATE).
 * Either may be NULL. */
int ecdna_ssa_ctx_download_snapshots(ecdna_ssa_ctx* c, ecdna_snapshot_t* meta, uint16_t* rows);
/* Per-replicate statistics of the last launch (needs ECDNA_FLAG_REP_STATS): out[n_replicates]. */
int ecdna_ssa_ctx_download_stats(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out);
/* The end-of-run subsample of the last launch (ABI v13; params.subsample_cells > 0, else ECDNA_E_STATE, as before a
 * launch). Either buffer may be NULL. out_stats[n_replicates]: the statistics of replicate i's sample, with the
 * definitions of ecdna_rep_stats_t (cells = the sample's size, distances against params.stats_target_hist).
 * out_sample_hist[n_param_sets * hist_bins]: per set, the sum of its replicates' sample histograms, binned as
 * out_hist (bin 0 = N- cells, last bin = overflow). Chunked runs are covered (the buffers are sized by the run, not
 * the chunk). ecdna_ssa_ctx_reduce does not reduce the sample histogram: callers sum the shards' themselves. */
int ecdna_ssa_ctx_download_sample(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats, uint64_t* out_sample_hist);
/* The per-snapshot statistics of the last launch (added within ABI v13; ecdna_ssa_ext_t.snapshot_stats, else
 * ECDNA_E_STATE, as before a launch, and as when a sample buffer is asked for with snapshot_subsample_cells == 0). Any
 * buffer may be NULL. out_stats[n_replicates][n_snapshots]: the statistics of replicate i's state at snapshot s;
 * out_sample_stats, same shape: those of its sample (cells = the sample's size). out_hist and out_sample_hist
 * [n_snapshots][n_param_sets][hist_bins]: per snapshot and set, the sum of the replicates' (samples') histograms,
 * binned as out_hist of ecdna_ssa_ctx_download. Chunked runs are covered. ecdna_ssa_ctx_reduce does not reduce these
 * histograms: callers sum the shards' themselves. */
int ecdna_ssa_ctx_download_snapshot_stats(ecdna_ssa_ctx* c, ecdna_rep_stats_t* out_stats,
                                          ecdna_rep_stats_t* out_sample_stats, uint64_t* out_hist,
                                          uint64_t* out_sample_hist);
/* ABC rejection on the GPU (added within ABI v13): a post-launch acceptance pass over the statistics a context already
 * holds on the device. abc.md §Implementation asks for thresholds that can be tuned after the expensive simulations
 * without re-running them: the statistics stay in HBM after a launch, so the pass may be called any number of times
 * after one launch, with different thresholds. The host receives only what it keeps — the per-set counts (the
 * posterior), a 4-byte mask per replicate, and the accepted replicates' ids and records — and a sharded sweep sums one
 * small integer array over the GPUs instead of gathering every record.
 *
 * The source: which statistics are tested, and its T timepoints. */
typedef enum {
    ECDNA_ACCEPT_FINAL = 0,            /* ecdna_ssa_ctx_download_stats' array, T = 1 */
    ECDNA_ACCEPT_SAMPLE = 1,           /* ecdna_ssa_ctx_download_sample's, T = 1 */
    ECDNA_ACCEPT_SNAPSHOTS = 2,        /* download_snapshot_stats' out_stats, T = n_snapshots */
    ECDNA_ACCEPT_SNAPSHOT_SAMPLES = 3, /* ... out_sample_stats, T = n_snapshots */
    ECDNA_ACCEPT_PASSAGES = 4,         /* download_passages' out_stats, T = n_passages */
    ECDNA_ACCEPT_PASSAGE_SAMPLES = 5,  /* ... out_sample_stats, T = n_passages */
    /* (6 and 7 are not sources: ECDNA_E_INVALID) */
    ECDNA_ACCEPT_COHORT = 8,           /* download_cohort's out_stats, T = n_targets: timepoint p is target p */
    ECDNA_ACCEPT_COHORT_SAMPLES = 9,   /* ... out_sample_stats, T = n_targets (needs sample_cells) */
    /* (10 and 11 are not sources: ECDNA_E_INVALID) */
    ECDNA_ACCEPT_RESCORED = 12,        /* download_rescored's records, T = the P of the last ecdna_ssa_ctx_rescore */
    ECDNA_ACCEPT_RESCORED_TIMEPOINTS   /* 13, the next value: download_rescored_timepoints' records, T = the context's
                                          timepoints (n_snapshots or n_passages) */
} ecdna_accept_source_t;
/* The rescored timepoints (source 13): the records lie [T][n] (rep stride 1, timepoint stride n). On a passage context
 * the error rule is the passage sources' (error stride n: error == 0 in the summary of every participating phase); on a
 * snapshot context the one-summary rule (error stride 0). ECDNA_E_STATE on a context without the timepoint keep block,
 * and before an ecdna_ssa_ctx_rescore_timepoints. */
/* The cohort sources: the error rule is the one-summary rule of ECDNA_ACCEPT_FINAL; the records lie [P][n] (rep stride 1,
 * timepoint stride n, error stride 0); timepoint_mask = 1 << p gives patient p's acceptance or quantiles, 0 all P
 * jointly, as for every source. A context without the cohort block returns ECDNA_E_STATE for both, and so does
 * ECDNA_ACCEPT_COHORT_SAMPLES without sample_cells. */

/* One threshold row: the largest accepted value of each of the four distances of ecdna_rep_stats_t. Each must be
 * >= 0 (not NaN); +inf switches that statistic off. */
typedef struct { double ks, mean_rel, entropy_rel, frequency_diff; } ecdna_accept_threshold_t;

/* Acceptance mapping v1. Replicate i of the call is accepted under threshold row q iff both hold:
 *  1. It is error-free: for the first four sources summaries[i].error == 0 (ecdna_ssa_ctx_download's summaries); for
 *     the passage sources error == 0 in the summary of every participating phase (ecdna_ssa_ctx_download_passages').
 *  2. For every participating timepoint t and each of the four distances x: thr[q].x == +inf, or d[i][t].x <= thr[q].x.
 *     A distance equal to its threshold passes. A NaN distance fails unless the threshold is +inf.
 * A snapshot that was not taken and an extinct phase need no special case: both are scored as an empty population
 * (ks = 1.0) already. */
typedef struct {
    uint32_t struct_size;        /* sizeof(ecdna_ssa_accept_t), else ECDNA_E_INVALID */
    uint32_t source;             /* ecdna_accept_source_t */
    uint32_t n_thresholds;       /* Q, 1 .. 32 */
    uint32_t list_threshold;     /* q < Q: the row whose accepted replicates are listed */
    const ecdna_accept_threshold_t* thresholds; /* host, [Q] */
    uint64_t timepoint_mask;     /* bit t = timepoint t takes part; 0 = all T */
    uint64_t list_capacity;      /* records the list may hold; 0 = no list */
    uint64_t reserved;           /* must be 0 */
} ecdna_ssa_accept_t;

/* Enqueue the acceptance pass on the stream of the last launch. Asynchronous; a later call replaces the results, a
 * relaunch invalidates them. The pass's buffers (mask, counts, workgroup counts, list) belong to the context: allocated
 * at the first call that needs them, grown by later ones, freed at destroy.
 * ECDNA_E_INVALID (the message names the field): NULL c or a, wrong struct_size, unknown source, n_thresholds outside
 * 1 .. 32, list_threshold >= n_thresholds, NULL thresholds, a threshold that is negative or NaN, timepoint_mask bits at
 * or above T, reserved != 0, n_replicates >= 2^32.
 * ECDNA_E_STATE: before a launch; the context does not hold the source's statistics (whenever the matching download
 * returns ECDNA_E_STATE); those statistics were computed without a target, so every distance is 0 and nothing could be
 * rejected.
 * ECDNA_E_NOMEM: the pass's buffers do not fit; the context stays usable and its other outputs intact. */
int ecdna_ssa_ctx_accept(ecdna_ssa_ctx* c, const ecdna_ssa_accept_t* a);
/* The results of the last ecdna_ssa_ctx_accept (ECDNA_E_STATE before one, and after a relaunch until the next).
 * Synchronises, as the other downloads do. Any pointer may be NULL.
 *  - out_counts[Q][n_param_sets]: accepted replicates of this call per threshold row and per global parameter set
 *    s = r / reps_per_set. Shards' arrays sum to the whole run's.
 *  - out_mask[n_replicates]: bit q is set iff replicate i is accepted under row q.
 *  - out_n_accepted: the number accepted under list_threshold — the whole count, even above list_capacity.
 *  - out_ids[list_capacity]: the global ids of the first min(n_accepted, list_capacity) accepted replicates, in
 *    ascending call order (i ascending): the order is part of the contract. Entries past them are not written.
 *  - out_list_stats[list_capacity][T]: the listed replicates' records of the source, all T timepoints in timepoint
 *    order (whatever timepoint_mask): byte for byte the rows of the corresponding download. */
int ecdna_ssa_ctx_download_accept(ecdna_ssa_ctx* c, uint64_t* out_counts, uint32_t* out_mask,
                                  uint64_t* out_n_accepted, uint64_t* out_ids,
                                  ecdna_rep_stats_t* out_list_stats);
/* Acceptance over repeated thinnings of the kept samples (added within ABI v13). Thinning mapping v1 reserves a draw
 * index d in 0 .. 63: 64 independent thinnings of one kept sample, and the share of them a replicate passes estimates
 * its acceptance probability under measurement noise — the weight of the simulation in ABC with measurement noise, the
 * mean of the acceptance indicator over the sampling of the patient's m1 cells. The call below counts that share in one
 * pass over the kept samples and keeps only the counts: no record is stored, no target slot is spent on a draw, and
 * several targets (two biopsies, every timepoint) are accepted jointly on each draw.
 *
 * Thinned acceptance mapping v1. A call names a store (timepoints = 0: the keep block's one slice; 1: the timepoint
 * keep block's T slices), target histograms, a number of measured cells per target, Q <= 32 threshold rows, a
 * timepoint mask and a draw range first_draw .. first_draw + n_draws - 1 inside 0 .. 63.
 *  - Keep store: n_targets = P in 1 .. 64 targets for the same slice; for acceptance they are the timepoints (T = P), as
 *    for source 12. Timepoint store: exactly one target per timepoint (n_targets == T), as for source 13.
 *  - For one draw d, every target is scored on the thinned sample that thinning mapping v1 defines for
 *    (sample_cells[slot], d). Nothing in that mapping changes: the same key per slice (seed, or seed_g), the same stream
 *    tag, the same grouping (targets with equal m1 see the same thinned sample), the same whole-sample rule when
 *    m1 >= a + b, the same guard records.
 *  - Replicate i passes row q on draw d iff acceptance mapping v1 accepts it on those records: rule 1 (errors) as source
 *    12 for the keep store and as source 13 for the timepoint store (on a passage context: per participating phase);
 *    rule 2 (distances) over the participating targets or timepoints. A tie passes, +inf switches a statistic off, a
 *    NaN fails.
 *  - passes[i][q], u8, laid out [n][Q]: the number of draws of the range that replicate i passes under row q (0 .. 64).
 *  - sums[Q][n_param_sets], u64: per row and GLOBAL parameter set, the sum of passes over the call's replicates.
 *    Integers: shards' arrays sum to the whole run's.
 *  - By construction passes[i][q] equals the sum over d of bit q of the mask that ecdna_ssa_ctx_rescore_sized /
 *    _rescore_timepoints_sized at draw d, followed by ecdna_ssa_ctx_accept on source 12 / 13 with the same thresholds
 *    and mask, would give. That equality is part of the contract: the records are never stored, but they are the same
 *    numbers (the same f64 operations in the same order), so a threshold that ecdna_ssa_ctx_select took from one draw's
 *    records cuts in exactly the same place.
 *  - Nothing depends on chunk, shard, grid or device.
 *
 * The call owns its buffers (target CDFs and scalars, passes, sums) and leaves untouched the rescored records of both
 * stores and their validity, the keys ecdna_ssa_ctx_select cached, the results of ecdna_ssa_ctx_accept and what
 * ecdna_ssa_ctx_pool_accepted* pool. It needs no earlier rescore. */
typedef struct {
    uint32_t struct_size;          /* sizeof(ecdna_ssa_accept_draws_t) */
    uint32_t timepoints;           /* 0: the keep block's store, 1: the timepoint keep block's */
    uint32_t n_targets;            /* keep store: P, 1 .. 64; timepoint store: T */
    const uint64_t* target_hists;  /* host [n_targets][hist_bins], no all-zero row */
    const uint32_t* sample_cells;  /* host [n_targets], required; each 1 .. keep_cells of the store */
    uint32_t first_draw;           /* first thinning draw of the range */
    uint32_t n_draws;              /* 1 .. 64, first_draw + n_draws <= 64 */
    uint32_t n_thresholds;         /* Q, 1 .. 32 */
    const ecdna_accept_threshold_t* thresholds; /* host, [Q] */
    uint64_t timepoint_mask;       /* bit t = target (keep store) or timepoint t takes part; 0 = all */
    uint64_t reserved;             /* must be 0 */
} ecdna_ssa_accept_draws_t;
/* Enqueue the pass on the stream of the last launch, as ecdna_ssa_ctx_accept does. Asynchronous; a later call replaces
 * the results, a relaunch invalidates them.
 * ECDNA_E_INVALID (the message names the field): NULL c or block, a wrong struct_size, reserved != 0, timepoints above 1,
 * n_targets outside 1 .. 64 or different from T on the timepoint store, NULL target_hists, an all-zero target row,
 * sample_cells NULL or an entry outside 1 .. keep_cells, n_draws outside 1 .. 64, first_draw + n_draws > 64,
 * n_thresholds outside 1 .. 32, NULL thresholds, a negative or NaN threshold, timepoint_mask bits at or above T,
 * n_replicates >= 2^32.
 * ECDNA_E_STATE: before a launch; a context without the named block.
 * ECDNA_E_NOMEM: the call's buffers do not fit; the context stays usable and its other outputs intact. */
int ecdna_ssa_ctx_accept_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a);
/* The results of the last ecdna_ssa_ctx_accept_draws (ECDNA_E_STATE before one, and after a relaunch until the next).
 * Synchronises. Either pointer may be NULL. out_sums [Q][n_param_sets], out_passes [n_replicates][Q]. */
int ecdna_ssa_ctx_download_accept_draws(ecdna_ssa_ctx* c, uint64_t* out_sums, uint8_t* out_passes);
/* The accepted thinnings pooled (added within ABI v13): the posterior predictive check of ABC with measurement noise.
 * ecdna_ssa_ctx_accept_draws gives a replicate its weight, the number of thinning draws it passes; this call pools what
 * was accepted. The pseudo-data that were actually accepted are the thinned samples of m1 cells on the passing draws:
 * their pooled histogram is the posterior predictive of the measurement itself. It is not the weighted pool of the kept
 * samples scaled by m1 / m: conditioning on "this draw passed" selects thinnings that resemble the target.
 *
 * Thinned pooling mapping v1.
 *  - The block means what it means for ecdna_ssa_ctx_accept_draws: the store (the keep block's one slice or the
 *    timepoint keep block's T slices), n_targets slots (the targets of the keep store, or one target per timepoint),
 *    sample_cells[slot], the draw range, the Q threshold rows and timepoint_mask. threshold is a row q < Q.
 *  - Verdict. Replicate i passes row q on draw d exactly when thinned acceptance mapping v1 says so: the error rule, the
 *    participating slots, ties, +inf, NaN and guard records that pass are all as in that mapping. Nothing of that mapping
 *    or of thinning mapping v1 changes.
 *  - out_thinned[slot][s], for every slot — slots the mask leaves out of the verdict are included: a held-out biopsy or
 *    timepoint is predicted, not conditioned on. It is the sum, over the call's replicates i of global set s and over
 *    the draws d of the range that i passes under row q, of the clipped histogram of the slot's scored sample on draw d:
 *    the sample thinning mapping v1 defines for (sample_cells[slot], d) on the slot's slice, under the same key, stream
 *    tag and draw index; when m1 >= a + b it is the whole kept sample, on every passing draw. Binning is that of
 *    ecdna_ssa_ctx_pool_accepted: bin 0 holds the N- cells, true copy numbers are clipped at hist_bins - 1. A guard
 *    header, a size the plan refuses and the 2^16-draw guard add nothing.
 *  - out_kept[slice][s], for every slice (n_slices is 1 on the keep store and T on the timepoint store): the sum over
 *    the replicates i of set s of passes[i][q] times the histogram of i's whole kept sample of the slice, binned the
 *    same way. A guard header adds nothing.
 *  - Contracts, equalities of integers.
 *    K1. out_kept equals the sum over d of ecdna_ssa_ctx_pool_accepted(q) (respectively _pool_accepted_timepoints(q))
 *        taken after the sized rescore at draw d and ecdna_ssa_ctx_accept on source 12 / 13 with the same thresholds and
 *        mask.
 *    K2. For a slot with sample_cells[slot] == keep_cells of its store, so that every replicate is scored whole,
 *        out_thinned[slot] equals out_kept[slice of the slot].
 *    K3. The bin sum of out_thinned[slot][s] equals the sum over i in s of passes[i][q] x min(sample_cells[slot],
 *        a_i + b_i), the term being 0 under a guard header; passes is that of ecdna_ssa_ctx_accept_draws with the same
 *        block.
 *    K4. Targets with equal m1 on one slice add the same thinned histograms to their rows.
 *    K5. Shards' arrays sum to the whole run's. Nothing depends on chunk, shard, grid or device.
 *
 * The call owns its buffers: target CDFs and scalars, and the two pooled arrays, (n_targets + n_slices) x n_param_sets x
 * hist_bins x 8 bytes, allocated at the first call, grown by later ones and freed at destroy. It needs neither an earlier
 * ecdna_ssa_ctx_accept_draws nor a rescore, and leaves untouched the results of ecdna_ssa_ctx_accept_draws and
 * ecdna_ssa_ctx_accept, the rescored records of both stores and their validity, the keys ecdna_ssa_ctx_select cached and
 * what ecdna_ssa_ctx_pool_accepted* pool. A relaunch invalidates nothing of this call: it holds no result.
 *
 * Synchronous, as ecdna_ssa_ctx_pool_accepted is; runs on the stream of the last launch. out_thinned: host
 * [n_targets][n_param_sets][hist_bins] or NULL; out_kept: host [n_slices][n_param_sets][hist_bins] or NULL; an output
 * that is NULL is not computed.
 * ECDNA_E_INVALID (the message names the field): everything ecdna_ssa_ctx_accept_draws refuses, with the same messages;
 * threshold >= n_thresholds; both outputs NULL.
 * ECDNA_E_STATE: before a launch; a context without the named block.
 * ECDNA_E_NOMEM: the call's buffers do not fit; the context stays usable and its other outputs intact. */
int ecdna_ssa_ctx_pool_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t threshold,
                             uint64_t* out_thinned, uint64_t* out_kept);
/* ABC thresholds on the GPU (added within ABI v13): exact order statistics of the four distances over the statistics a
 * context already holds, so that "keep the closest 1 % of the runs" needs neither a download of every record nor, on
 * several GPUs, a gather of them. An 8-bit radix select: each of eight passes leaves a small integer histogram, and
 * shards' histograms sum exactly, as the counts of ecdna_ssa_ctx_accept do.
 *
 * Select mapping v1.
 *  - Source, timepoints, population. The source is an ecdna_accept_source_t; its T timepoints, timepoint_mask (0 = all)
 *    and strides mean what they mean for ecdna_ssa_ctx_accept. The population is the replicates that rule 1 of
 *    acceptance mapping v1 calls error-free (error == 0 in the one summary, or, for the passage sources, in the summary
 *    of every participating phase), pooled over all parameter sets of the call. Its size is M.
 *  - Key. Of a distance value d: -0.0 becomes +0.0 and any NaN the canonical quiet NaN, bits 0x7FF8000000000000; then
 *    key(d) = bits(d) ^ 0x8000000000000000 when the sign bit is clear and ~bits(d) when it is set: the usual
 *    order-preserving map, and NaN sorts above +inf. Replicate i's key for distance x is the maximum, over the
 *    participating timepoints t, of key(d[i][t].x): a replicate passes threshold v on x at every participating
 *    timepoint iff key_x[i] <= key(v).
 *  - Order statistic. For rank k >= 1 and distance x, value_x(k) is the number whose key is the k-th smallest of the M
 *    keys, and counts_le_x(k) the number of the M keys <= that key: >= k, and > k on a tie. For k > M, and for every k
 *    when M = 0, value = +inf and counts_le = M (+inf switches a statistic off in accept, which then accepts all M). A
 *    NaN value means that fewer than k replicates have a number for that distance; it is reported as NaN and must not
 *    be fed to accept.
 *  - Consequence, part of the contract. For a finite value_x(k), ecdna_ssa_ctx_accept with that threshold on x and +inf
 *    on the other three, on the same source and timepoint_mask, accepts exactly counts_le_x(k) replicates, and no
 *    smaller threshold accepts k or more.
 *  - Ranks from fractions. f in (0, 1] maps to k = max(1, (uint64)ceil(f * (double)M)), evaluated in f64.
 * The distance order is that of ecdna_accept_threshold_t: ks, mean_rel, entropy_rel, frequency_diff. */
typedef struct {
    uint32_t struct_size;        /* sizeof(ecdna_ssa_select_t), else ECDNA_E_INVALID */
    uint32_t source;             /* ecdna_accept_source_t */
    uint64_t timepoint_mask;     /* bit t = timepoint t takes part; 0 = all T */
    uint32_t n_ranks;            /* K, 1 .. 32 */
    uint32_t reserved;           /* must be 0 */
    const uint64_t* ranks;       /* host, [K], each >= 1; or NULL */
    const double* fractions;     /* host, [K], each in (0, 1]; or NULL: exactly one of the two is given */
} ecdna_ssa_select_t;

/* The order statistics of one context's replicates: eight digit passes and the walk over their histograms. Synchronous,
 * as the downloads are; any output may be NULL. out_population: M. out_ranks[K]: the ranks (those given, or those the
 * fractions map to). out_values[4][K] and out_counts_le[4][K]: value_x(k_j) and counts_le_x(k_j).
 * Both calls keep scratch that belongs to the context (the keys, 32 bytes per replicate, and one pass's histogram):
 * allocated at the first call, freed at destroy. The keys are kept between passes and calls for one (source,
 * timepoint_mask) and dropped by a relaunch. The results of ecdna_ssa_ctx_accept are not touched.
 * ECDNA_E_INVALID (the message names the field): NULL c or s, wrong struct_size, unknown source, n_ranks outside 1 .. 32,
 * both or neither of ranks and fractions, a rank of 0, a fraction outside (0, 1] or NaN, timepoint_mask bits at or above
 * T, reserved != 0, n_replicates >= 2^32; for select_digits also pass > 7, n_prefixes outside 1 .. 32, NULL prefixes or
 * out_hist.
 * ECDNA_E_STATE: exactly where ecdna_ssa_ctx_accept returns it (before a launch; a source the context does not hold;
 * statistics computed without a target).
 * ECDNA_E_NOMEM: the scratch does not fit; the context stays usable and its other outputs intact. */
int ecdna_ssa_ctx_select(ecdna_ssa_ctx* c, const ecdna_ssa_select_t* s, uint64_t* out_population,
                         uint64_t* out_ranks, double* out_values, uint64_t* out_counts_le);
/* One pass of the select, the shard primitive: out_hist[4][K][256], where out_hist[x][j][d] counts the population's
 * keys of distance x whose top 8 * pass bits equal those of prefixes[x][j] (host, [4][K]; lower bits are ignored) and
 * whose next 8 bits are d. Pass 0 counts everything, so the sum of any row is M. Shards' arrays sum to the whole
 * run's: a sharded sweep sums each pass's array over its GPUs, walks it to the next pass's prefixes (per row: the
 * smallest digit whose cumulative count reaches the remaining rank) and finds the global order statistics with eight
 * small all-reduces instead of a gather of every record. Synchronous. */
int ecdna_ssa_ctx_select_digits(ecdna_ssa_ctx* c, uint32_t source, uint64_t timepoint_mask, uint32_t pass,
                                uint32_t n_prefixes, const uint64_t* prefixes, uint64_t* out_hist);
/* ABC thresholds over thinning draws (added within ABI v13). ecdna_ssa_ctx_accept_draws and ecdna_ssa_ctx_pool_draws
 * take threshold rows; ecdna_ssa_ctx_select finds thresholds, but over stored records, the records of one draw. In ABC
 * with measurement noise the population a quantile cuts is the pseudo-datasets, the pairs (replicate, draw): "keep the
 * closest 1 %" is the rank ceil(0.01 x M) order statistic over all of them, and with it sum(passes) / M is the
 * acceptance rate that was asked for. The calls below find it in one pass of the thinning core and the eight digit
 * passes of ecdna_ssa_ctx_select, without storing a record.
 *
 * Thinned select mapping v1.
 *  - Block. ecdna_ssa_accept_draws_t means what it means for ecdna_ssa_ctx_accept_draws — the store, the slots,
 *    sample_cells, the draw range, timepoint_mask — except that it carries no threshold rows: n_thresholds must be 0 and
 *    thresholds NULL. n_replicates x n_draws must be below 2^32: the digit pass indexes its keys with 32 bits.
 *  - Population. The pairs (i, d): replicate i error-free under rule 1 of thinned acceptance mapping v1 (the one-summary
 *    rule on the keep store and on a snapshot context; on a passage context the rule per participating phase), draw d in
 *    first_draw .. first_draw + n_draws - 1. Its size is M = (error-free replicates) x n_draws.
 *  - Key. key_x(i, d) is the maximum, over the participating slots, of select mapping v1's key of distance x of the
 *    record thinned acceptance mapping v1 scores for that slot on draw d: the same key per slice, stream tag and
 *    grouping, the same f64 operations in the same order, the same whole-sample rule when m1 >= a + b (one record,
 *    counted on every draw). A guard record (the header's, the size's, the 2^16 draws') has four zero distances and so
 *    the key of 0.0. Nothing of thinning mapping v1 or of thinned acceptance mapping v1 changes.
 *  - Order statistics, ranks from fractions, over-rank (value +inf, counts_le = M) and the reporting of NaN are exactly
 *    select mapping v1's, over these M keys. Ranks are u64; M can reach 2^32.
 *  - Contracts, all equalities of integers or of bits.
 *    S1. ecdna_ssa_ctx_select_draws_digits(block, pass, prefixes) equals the sum, over the draws d of the range, of
 *        ecdna_ssa_ctx_select_digits(source 12 or 13, timepoint_mask, pass, prefixes) taken after the sized rescore at
 *        draw d (ecdna_ssa_ctx_rescore_sized or _rescore_timepoints_sized with the same targets and sizes). So
 *        ecdna_ssa_ctx_select_draws equals select mapping v1's walk over the union of those keys.
 *    S2. For a finite value_x(k), ecdna_ssa_ctx_accept_draws with the same block and one row — that value on x, +inf on
 *        the other three — gives sums[0] that, summed over the sets, equal counts_le_x(k); no smaller threshold reaches k.
 *    S3. With n_draws = 1 the four outputs are bit for bit those of ecdna_ssa_ctx_select on source 12 or 13 after the
 *        sized rescore at that draw.
 *    S4. Shards' digit arrays sum to the whole run's. Nothing depends on chunk, shard, grid or device.
 *
 * The calls own their buffers: the keys, [4][n_replicates x n_draws] u64 (32 x n x n_draws bytes: 2.1 GB at n = 2^20 and
 * 64 draws), one pass's histogram, the target CDFs and scalars; allocated at the first call, grown by later ones, freed at
 * destroy. ecdna_ssa_ctx_select_draws makes the keys once and its eight passes over them.
 * ecdna_ssa_ctx_select_draws_digits makes them in pass 0, and the context remembers the block they were made for (its
 * fields, and copies of target_hists and sample_cells): a pass above 0 whose block differs, or that follows a relaunch,
 * returns ECDNA_E_STATE — pass 0 of the same block must come first. The calls leave untouched the keys and validity of
 * ecdna_ssa_ctx_select, the rescored records of both stores, and the results of ecdna_ssa_ctx_accept,
 * ecdna_ssa_ctx_accept_draws and ecdna_ssa_ctx_pool_draws. They need no earlier rescore.
 *
 * Both are synchronous, as ecdna_ssa_ctx_select and _select_digits are, and run on the stream of the last launch.
 * ranks, fractions and n_ranks (K) follow the rules of ecdna_ssa_select_t; pass, n_prefixes, prefixes and out_hist those
 * of ecdna_ssa_ctx_select_digits. Any output of ecdna_ssa_ctx_select_draws may be NULL.
 * ECDNA_E_INVALID (the message names the field): everything ecdna_ssa_ctx_accept_draws refuses, with the same messages,
 * but for its threshold rules; select_draws.n_thresholds != 0 or select_draws.thresholds != NULL; n_replicates x n_draws
 * >= 2^32; n_ranks outside 1 .. 32, both or neither of ranks and fractions, a rank of 0, a fraction outside (0, 1] or
 * NaN; pass > 7, n_prefixes outside 1 .. 32, NULL prefixes or out_hist.
 * ECDNA_E_STATE: before a launch; a context without the named block; a pass above 0 without pass 0 of the same block.
 * ECDNA_E_NOMEM: a buffer does not fit (the message carries its bytes; a narrower draw range needs fewer); the context
 * stays usable and its other outputs intact. */
int ecdna_ssa_ctx_select_draws(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a,
                               uint32_t n_ranks, const uint64_t* ranks, const double* fractions,
                               uint64_t* out_population, uint64_t* out_ranks,
                               double* out_values /* [4][K] */, uint64_t* out_counts_le /* [4][K] */);
int ecdna_ssa_ctx_select_draws_digits(ecdna_ssa_ctx* c, const ecdna_ssa_accept_draws_t* a, uint32_t pass,
                                      uint32_t n_prefixes, const uint64_t* prefixes /* [4][K] */,
                                      uint64_t* out_hist /* [4][K][256] */);
/* Reference draws (ECDNA_FLAG_REFERENCE_DRAWS, ABI v7): per replicate, the number of 32-bit words its ChaCha8
 * stream (seed_from_u64(seed), stream seed*10 + r) had handed out when it stopped — where the reference's
 * end-of-run subsampling continues the same rng (into_subsampled(nb, &mut rng), src/main.rs:110-123, 184-197;
 * ecdna_host_subsample_reference). out[n_replicates]. */
int ecdna_ssa_ctx_download_rng_words(ecdna_ssa_ctx* c, uint64_t* out);
/* Row stride (cells) of the rows buffer, or 0 when the run is chunked (rows not downloadable). */
int64_t ecdna_ssa_ctx_row_stride(const ecdna_ssa_ctx* c);
/* Replicates per chunk (memory bound) and lanes of the persistent stepper grid. */
int ecdna_ssa_ctx_geometry(const ecdna_ssa_ctx* c, uint64_t* chunk_replicates, uint64_t* grid_lanes);

/* The kernel instance a context launches (ABI v7): every choice ecdna_ssa_ctx_create makes from the
 * workload shape and the ECDNA_SSA_* environment knobs, so that a benchmark line can name
 * the instance it timed and a flip of an automatic rule shows up in its output. Results never depend on
 * any of these; they are speed choices. */
typedef enum {
    ECDNA_KERNEL_ROWS = 0,       /* ssa_stepper: the row store (one u16 per cell in HBM) */
    ECDNA_KERNEL_BINS = 1,       /* ssa_stepper_bins: the bin store (ECDNA_FLAG_BIN_STORE) */
    ECDNA_KERNEL_REFDRAWS = 2    /* ssa_stepper_refdraws: the reference draws (ECDNA_FLAG_REFERENCE_DRAWS) */
} ecdna_kernel_kind_t;
typedef struct {
    int32_t kernel;            /* ecdna_kernel_kind_t */
    int32_t schedule;          /* bin stepper: 0 occupancy-first, 1 max-ILP, 2 occupancy-first capped at 128
                                  VGPRs (K = 64 / u16), 3 max-ILP with paired lanes; -1 for the other kernels */
    int32_t paired;            /* 1: lane l < 32 owns a replicate, lane l + 32 helps its N- fast-forward (pairs) */
    int32_t rotation;          /* number of chunks whose replicates rotate through the lanes */
    int32_t rot_tick_log2;     /* rotation tick (loop iterations, log2) */
    int32_t drain_control;     /* number of chunks whose youngest wave slots stop admitting replicates early */
    int32_t cost_order;        /* 1: replicates start costliest set first (params.set_cost_hint) */
    int32_t runtime_flags;     /* 1: the instance reads f32 time, the event hash and snapshots from its arguments
                                  (TF = 1); 0: compiled out */
    uint32_t bin_kmax;         /* bin store: binned copy numbers (0 for the other kernels) */
    uint32_t bin_c32;          /* bin store: 1 = u32 counters, 0 = u16 */
    uint32_t block_lanes;      /* workgroup size */
    uint32_t blocks_per_cu;    /* workgroups per CU of the launched grid (rounded up; largest chunk) */
    uint32_t cus;              /* compute units of the device */
    uint32_t n_chunks;         /* launches per run (HBM-bounded chunks) */
    uint32_t vgprs;            /* per lane, as compiled (hipFuncGetAttributes numRegs) */
    uint32_t lds_bytes;        /* static LDS per workgroup */
    uint32_t scratch_bytes;    /* private segment per lane */
    uint32_t window;           /* row store: 1 = LDS tail window variant */
    uint64_t chunk_replicates; /* replicates per chunk */
    uint64_t grid_lanes;       /* lanes of the launched grid (largest chunk; <= the occupancy cap) */
} ecdna_ssa_instance_t;
int ecdna_ssa_ctx_instance(const ecdna_ssa_ctx* c, ecdna_ssa_instance_t* out);
int ecdna_ssa_ctx_destroy(ecdna_ssa_ctx* c);

/* ---- Multi-GPU reduction (ABI v6; RCCL over xGMI).
 * Replicates shard over GPUs by GLOBAL id (first_replicate / replicate_stride), so every shard draws exactly
 * the streams the same replicates draw in one big run, and the whole run's histogram and totals are the
 * element-wise sum of the shards' — one all-reduce (ncclUint64, ncclSum), exact and order-independent. This
 * replaces the reference's collection of per-replicate results from its rayon loop (src/main.rs:221-224)
 * when the replicates live on several GPUs.
 * A communicator is an RCCL ncclComm_t passed as void*: made here (ecdna_ssa_comm_init_all for one process
 * driving several devices, one host thread per device; ecdna_ssa_comm_init_rank for one process per device
 * with the unique id of ecdna_ssa_comm_unique_id shared by the caller), or made by the caller with RCCL. RCCL
 * (librccl.so.1) is loaded at the first of these calls; without it they return ECDNA_E_COMM. */
#define ECDNA_COMM_ID_BYTES 128
int ecdna_ssa_comm_unique_id(uint8_t out_id[ECDNA_COMM_ID_BYTES]);
int ecdna_ssa_comm_init_rank(const uint8_t id[ECDNA_COMM_ID_BYTES], int n_ranks, int rank, int device,
                             void** out_comm);
/* out_comms[n_devices]: one communicator per device of devices[] (ncclCommInitAll). */
int ecdna_ssa_comm_init_all(int n_devices, const int* devices, void** out_comms);
int ecdna_ssa_comm_destroy(void* comm);
/* In-place all-reduce (sum) over `comm` of a run's DEVICE histogram [n_param_sets * hist_bins] u64 and totals
 * [n_param_sets], enqueued on `stream` (a hipStream_t; NULL = default). Every rank of the communicator must
 * call it with the same n_param_sets and hist_bins. Asynchronous. */
int ecdna_ssa_reduce_hist(void* comm, uint64_t* d_hist, ecdna_totals_t* d_totals, uint32_t n_param_sets,
                          uint32_t hist_bins, void* stream);
/* The same on a context's current outputs (ecdna_ssa_ctx_set_outputs or its own), on the stream of its last
 * launch; ecdna_ssa_ctx_download then returns the reduced histogram and totals. */
int ecdna_ssa_ctx_reduce(ecdna_ssa_ctx* c, void* comm);

#ifdef __cplusplus
}
#endif

#endif /* ECDNA_SSA_H */
