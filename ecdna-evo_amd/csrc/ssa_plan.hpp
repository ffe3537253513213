// ssa_plan.hpp — what ecdna_ssa_ctx_create decides about a run's launches, as one pure function: the chunk size, the
// bin stepper's schedule and lane pairing, the persistent grid, replicate rotation and the drain control. Host code
// without a HIP runtime call: plan_launch computes a LaunchPlan from the run's shape (RunShape: what the parameters
// decide), the device's facts (DeviceFacts: what ssa_api.cpp asked the runtime) and the tuning knobs (Knobs: the
// ECDNA_SSA_* environment, read once per create), so that every rule can be walked on a machine without a GPU
// (tests/native/plan_check.cpp, tests/test_launch_plan.py). None of these decisions changes a result, only speed.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "ssa_launch.h"

namespace ecdna {
namespace plan {

// ---- the tuning knobs (INTEGRATION.md §6 lists them; tests/test_integration_doc.py holds the two together) ----

enum KnobId {
    C32,            // 1 forces u32 bin counters at any K: a development knob, results are the same
    MAX_ROW_BYTES,  // testing: the chunk budget in bytes (0 = 85 % of the free memory)
    MAX_CHUNK,      // testing: replicates per chunk at most (0 = what fits)
    WINDOW,         // row store: 0 selects the HBM-only variant of the LDS tail window stepper
    SCHED,          // bin stepper build: 0 default, 1 max-ILP, 2 auto, 3 the 128-VGPR build (K = 64 / u16; else 0)
    PAIR,           // paired lanes: 0 off, 1 whenever possible, 2 auto
    BLOCKS_PER_CU,  // workgroups per CU of the persistent grid (0 = the occupancy)
    MAX_BLOCKS,     // testing: force lane refill (0 = no cap)
    ROTATE,         // replicate rotation: 0 off, 1 on whenever possible, 2 auto
    ROT_TICK,       // log2 loop iterations between rotation ticks (at most 30)
    ROT_PARK_MIN,   // park at a tick only while this many replicates wait (unset: 1.5 partition grids)
    ADMIT,          // 0: no drain control
    ADMIT_SLOTS,    // wave slots per SIMD the drain control closes
    ADMIT_X8,       // eighths of a grid left when it closes them (tuning)
    kKnobCount
};
struct KnobDef {
    const char* name;
    uint64_t dflt;  // (ROT_PARK_MIN: its default depends on the grid, so the rule asks is_set)
};
constexpr KnobDef kKnobDefs[kKnobCount] = {
    {"ECDNA_SSA_C32", 0},           {"ECDNA_SSA_MAX_ROW_BYTES", 0}, {"ECDNA_SSA_MAX_CHUNK", 0},
    {"ECDNA_SSA_WINDOW", 1},        {"ECDNA_SSA_SCHED", 2},         {"ECDNA_SSA_PAIR", 2},
    {"ECDNA_SSA_BLOCKS_PER_CU", 0}, {"ECDNA_SSA_MAX_BLOCKS", 0},    {"ECDNA_SSA_ROTATE", 2},
    {"ECDNA_SSA_ROT_TICK", 10},     {"ECDNA_SSA_ROT_PARK_MIN", 0},  {"ECDNA_SSA_ADMIT", 1},
    {"ECDNA_SSA_ADMIT_SLOTS", 1},   {"ECDNA_SSA_ADMIT_X8", 12},
};

struct Knobs {
    uint64_t value[kKnobCount];
    bool is_set[kKnobCount];
    Knobs() {
        for (int k = 0; k < kKnobCount; ++k) {
            value[k] = kKnobDefs[k].dflt;
            is_set[k] = false;
        }
    }
    uint64_t operator[](KnobId k) const { return value[k]; }
    // a variable's text as the environment holds it: nullptr or empty leaves the default, else strtoull
    void parse(int k, const char* text) {
        if (!text || !*text) return;
        value[k] = std::strtoull(text, nullptr, 10);
        is_set[k] = true;
    }
};

// The only place the library reads its environment, once per create.
inline Knobs knobs_from_env() {
    Knobs k;
    for (int i = 0; i < kKnobCount; ++i) k.parse(i, std::getenv(kKnobDefs[i].name));
    return k;
}

// ---- the inputs ----

// What the runtime says about the device and the kernels of the run's shape (workgroups per CU by
// hipOccupancyMaxActiveBlocksPerMultiprocessor at the shape's block size; 0 = the shape has no such instance).
struct DeviceFacts {
    int cus = 0;
    int xccs = 0;  // 0: the query failed
    uint64_t free_bytes = 0;  // after the run-sized outputs are allocated, before the chunk's buffers
    int occ_rows = 0;         // the row stepper (its window variant and flags)
    int occ_refdraws = 0;     // the reference-draws stepper
    int occ_bins[4] = {0, 0, 0, 0};  // the bin stepper per schedule: 0 default, 1 max-ILP, 2 128-VGPR, 3 paired lanes
};

// What the parameters and the extension blocks decide.
struct RunShape {
    uint64_t n = 0;  // replicates of the run
    int process = 0;
    uint32_t kernel_flags = 0;  // the caller's flags and the internal bits (kFlagSnapshotsRt, kFlagPassageRt)
    uint32_t max_workgroups = 0;
    bool hinted = false;  // a cost hint orders the replicates' starts (set_cost_hint, n > 0)
    bool refdraws = false;
    // the cell store: bin_k binned copy numbers (0 = row store), u32 counters, the workgroup size of the stepper
    // (the kernels' own: bin_stepper_block, refdraws_block, else kStepperBlock; the caller sets it)
    uint32_t bin_k = 0;
    int bin_c32 = 0;
    uint32_t stepper_block = kStepperBlock;
    uint64_t row_stride = 0;  // device rows (the bin store: its large-k rows, big_cap cells)
    uint64_t out_stride = 0;  // downloaded and snapshot rows (cell_cap cells)
    uint32_t big_cap = 0;     // bin store: large-k row capacity
    uint32_t n_snapshots = 0;
    bool snap_rows_local = false;  // the snapshot rows are one chunk's scratch, not the run's
    uint32_t n_passages = 0;
    uint64_t founder_stride = 0;
    // bytes of one replicate's bin counters, and of everything a replicate of a chunk holds on the device: its row,
    // its bin counters, its parked scalars and state word (bin store: kParkVecs * 16 + 4), its snapshot rows where
    // they are the chunk's scratch, its founders in a passage run
    uint64_t bag_bytes = 0;
    uint64_t rep_bytes = 0;
};

inline uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

// The shape of a validated run. snap_stats: per-snapshot statistics are on (ecdna_ssa_ext_t); n_passages = 0: no
// passage block. stepper_block is left at kStepperBlock for the caller to set.
inline RunShape run_shape(const ecdna_ssa_params_t& p, bool snap_stats, uint32_t n_passages, uint32_t passage_cells,
                          const Knobs& knobs) {
    RunShape s;
    s.n = p.n_replicates;
    s.process = p.process;
    s.kernel_flags = p.flags | (p.n_snapshots ? kFlagSnapshotsRt : 0u) | (n_passages ? kFlagPassageRt : 0u);
    s.max_workgroups = p.max_workgroups;
    s.hinted = p.set_cost_hint && p.n_replicates;
    s.refdraws = (p.flags & ECDNA_FLAG_REFERENCE_DRAWS) != 0;
    s.n_snapshots = p.n_snapshots;
    s.n_passages = n_passages;
    if (n_passages) s.founder_stride = round_up(passage_cells, 64);
    s.row_stride = round_up(p.cell_cap, 64);
    s.out_stride = s.row_stride;
    if (p.flags & ECDNA_FLAG_BIN_STORE) {
        s.big_cap = (p.big_cap && p.big_cap < p.cell_cap) ? p.big_cap : p.cell_cap;
        s.row_stride = round_up(s.big_cap, 64);
        s.bin_k = p.bin_kmax ? p.bin_kmax : 64;
        // u16 counters hold at most 65535 cells per bin/group; K = 32 always uses u32 counters: the same LDS
        // footprint as K = 64/u16 (144 B per lane), no 16-bit packing in the updates and the scan (C3:
        // 119 ms against 126 ms with u16)
        s.bin_c32 = (p.cell_cap > 65535u || s.bin_k <= 32 || knobs[C32]) ? 1 : 0;
        s.bag_bytes = (uint64_t)s.bin_k * (s.bin_c32 ? 4u : 2u);
    }
    // (snapshot statistics without the run's snapshot rows, which ECDNA_FLAG_SNAPSHOT_ROWS allocates for n > 0: the
    // snapshot rows are the chunk's scratch, n_snapshots rows of out_stride cells per replicate of the chunk, so a
    // large run chunks instead of failing)
    s.snap_rows_local = snap_stats && !(p.n_snapshots && p.n_replicates && (p.flags & ECDNA_FLAG_SNAPSHOT_ROWS));
    const uint64_t rot_bytes = s.bin_k ? kParkVecs * 16u + 4u : 0u;  // parked scalars + state word
    const uint64_t snap_row_bytes = s.snap_rows_local ? p.n_snapshots * s.out_stride * sizeof(uint16_t) : 0u;
    // (a passage run: the chunk's founders, one row of passage_cells and {n-, n+} per replicate)
    const uint64_t founder_bytes = n_passages ? s.founder_stride * sizeof(uint16_t) + sizeof(uint2) : 0u;
    s.rep_bytes = s.row_stride * sizeof(uint16_t) + s.bag_bytes + rot_bytes + snap_row_bytes + founder_bytes;
    return s;
}

// ---- the plan ----

struct ChunkPlan {
    uint64_t first = 0;  // local index of the first replicate
    uint32_t n = 0;
    uint32_t blocks = 1;     // persistent grid of the chunk
    uint32_t rot_n_pad = 0;  // replicate rotation (bin store; 0 = off): partition size
    // drain control (admit_slot 0xffffffff: off)
    uint32_t admit_slot = 0xffffffffu;
    uint32_t admit_remaining = 0;
};

struct LaunchPlan {
    uint64_t chunk_reps = 0;  // replicates the chunk's buffers hold; 0: one replicate does not fit in the budget
    std::vector<ChunkPlan> chunks;  // they tile [0, n)
    int window = 1;    // LDS tail window stepper (0: the HBM-only variant)
    int schedule = 0;  // the bin stepper's: 0 default, 1 max-ILP (lone waves), 2 128-VGPR K = 64, 3 max-ILP paired lanes
    uint32_t stepper_block = kStepperBlock;
    uint32_t stepper_blocks_cap = 0;
    uint32_t rot_tick_log2 = 10;
    bool any_rotation = false;
    int32_t rot_park_min = 0;    // (any_rotation only)
    uint64_t rot_n_pad_max = 0;  // (any_rotation only) flags per partition the rotation buffers hold
};

// Partition x's replicates of a chunk of n under rotation (r = x mod kRotParts): its waiting and fresh counters start
// there.
inline int rot_part_count(uint32_t n, uint32_t x) { return x < n ? (int)((n - x + kRotParts - 1) / kRotParts) : 0; }

// The bin stepper's instruction-schedule rule, a pure function of the run's shape and the kernels'
// occupancies so that the CPU tests can walk any shape through it (ecdna_dev_bin_schedule, tests/test_host.py).
// Returns ecdna_ssa_instance_t.schedule: 0 occupancy-first, 1 max-ILP, 2 the 128-VGPR build (K = 64 / u16), 3 max-ILP
// paired lanes. pair_ok: birth-death without snapshots and a paired instance exists; pair_mode ECDNA_SSA_PAIR (0 off,
// 1 pairs whenever possible, 2 auto); sched ECDNA_SSA_SCHED (0, 1, 2 auto, 3);
// max_chunk the largest chunk's replicates; occ_def / occ_ilp workgroups per CU of the two builds.
inline int bin_schedule_rule(bool pair_ok, uint64_t pair_mode, uint64_t sched, uint64_t max_chunk, uint32_t cus,
                             bool k64u16, bool tf0, int occ_def, int occ_ilp, uint32_t stepper_block) {
    if (pair_ok && (pair_mode == 1 ||
                    (pair_mode == 2 && sched == 2 && max_chunk <= (uint64_t)cus * (ecdna::kStepperBlock / 2))))
        return 3;
    if (sched == 1 || (sched == 2 && max_chunk <= (uint64_t)cus * 256u)) return 1;
    if (k64u16 && (sched == 3 || (sched == 2 && tf0 && max_chunk >= 4ull * cus * 4u * ecdna::kStepperBlock))) return 2;
    if (sched == 2 && (occ_ilp >= occ_def || max_chunk < 4ull * (uint64_t)occ_def * cus * stepper_block)) return 1;
    return 0;
}

inline LaunchPlan plan_launch(const RunShape& s, const DeviceFacts& f, const Knobs& knobs) {
    LaunchPlan pl;
    pl.stepper_block = s.stepper_block;
    pl.window = knobs[WINDOW] ? 1 : 0;
    pl.rot_tick_log2 = (uint32_t)std::min<uint64_t>(knobs[ROT_TICK], 30);

    // chunks: one u16 row (and the rest of rep_bytes) per replicate of the chunk; chunk bounded by free HBM
    uint64_t budget = (uint64_t)((double)f.free_bytes * 0.85);
    if (knobs[MAX_ROW_BYTES]) budget = std::min<uint64_t>(budget, knobs[MAX_ROW_BYTES]);
    uint64_t fit = budget / s.rep_bytes;
    if (knobs[MAX_CHUNK]) fit = std::min<uint64_t>(fit, knobs[MAX_CHUNK]);
    if (fit == 0) return pl;  // (chunk_reps 0: one replicate row does not fit)
    pl.chunk_reps = std::min<uint64_t>(std::max<uint64_t>(s.n, 1), fit);
    const uint64_t n_chunks = s.n ? (s.n + pl.chunk_reps - 1) / pl.chunk_reps : 0;
    uint64_t max_chunk = 0;
    for (uint64_t k = 0; k < n_chunks; ++k) {
        ChunkPlan ch;
        ch.first = k * pl.chunk_reps;
        ch.n = (uint32_t)std::min<uint64_t>(pl.chunk_reps, s.n - ch.first);
        max_chunk = std::max<uint64_t>(max_chunk, ch.n);
        pl.chunks.push_back(ch);
    }

    // persistent stepper grid: as many resident lanes as the occupancy allows; the bin stepper's instruction schedule
    int per_cu = 0;
    if (s.refdraws) {
        per_cu = f.occ_refdraws;
    } else if (s.bin_k) {
        // Instruction schedule: with at most one wave of replicates per SIMD (every chunk within 256 lanes
        // per CU) each wave runs alone and waits on its own dependencies, and the max-ILP schedule is faster
        // (C2 8.6 -> 8.1 ms, C5 8-GPU shard 22.0 -> 21.1 s); with more, issue binds and the default schedule
        // keeps 4 waves per SIMD (max-ILP: 3, C3 +8 %). The K = 64 / u16 kernel needs 130 VGPRs (3
        // workgroups per CU); its 128-VGPR build fits 4 and pays once lanes run many replicates each (the
        // whole C4 sweep on one GPU, 16 per lane: 834 -> 771 ms) but not with few (C4 8-GPU shard, 2 per
        // lane: a longer drain, 127 -> 134 ms), so auto takes it from 4 replicates per lane of its grid on.
        // ECDNA_SSA_SCHED = 0 default, 1 max-ILP, 2 auto, 3 the 128-VGPR build (K = 64 / u16; else 0).
        // (auto only without f32 time and the event hash: that variant spills 12 B at 128 VGPRs)
        const bool k64u16 = s.bin_k == 64 && !s.bin_c32;
        const bool tf0 = (s.kernel_flags & kRuntimeFlagMask) == 0;
        // Where the max-ILP build keeps the default's occupancy (LDS bounds both: K = 32 / u32 and K = 64 / u32
        // since the f32 draw mapping v6, K = 256) it is taken too: its schedule then costs no lanes (C3 78.3 ->
        // 77.3 ms, C5 whole 31.9 -> 30.4 s, same box). With fewer than four replicates per lane of the default
        // grid it is taken even at one workgroup per CU less (K = 64 / u16, 118 against 134 VGPRs since v6: the
        // C4 8-GPU shard, two replicates per lane, 127 -> 119 ms), as the drain of the last replicates is
        // latency-bound (profiles/r04d_v6_suite_and_sched_sweep.txt).
        // Paired lanes: with at most half a wave of replicates per SIMD (the C5 8-GPU shard) the
        // idle half of each wave computes the next event's Philox block and soft log in the N- fast-forward.
        // Birth-death without snapshots (the fast-forward's domain). ECDNA_SSA_PAIR = 0 off, 1 whenever
        // possible, 2 auto.
        const bool pair_ok = s.process == ECDNA_BIRTH_DEATH && s.n_snapshots == 0 && f.occ_bins[3] != 0;
        pl.schedule = bin_schedule_rule(pair_ok, knobs[PAIR], knobs[SCHED], max_chunk, (uint32_t)f.cus, k64u16, tf0,
                                        f.occ_bins[0], f.occ_bins[1], s.stepper_block);
        // bin store: LDS-resident events, bounded by issue and LDS latency: every resident block helps
        per_cu = f.occ_bins[pl.schedule];
    } else {
        // Memory-level parallelism of the random row accesses saturates HBM at about 3 resident 256-lane
        // blocks per CU (C3 sweep, DESIGN.md §8: 1/2/3/4/7 blocks -> 617/372/329/336/349 ms); fewer
        // lanes also mean more replicates per lane and a shorter drain once the work queue is empty.
        per_cu = std::min(f.occ_rows, 3);
    }
    if (knobs[BLOCKS_PER_CU]) per_cu = (int)knobs[BLOCKS_PER_CU];
    if (per_cu < 1) per_cu = 1;
    pl.stepper_blocks_cap = (uint32_t)(per_cu * f.cus);
    if (s.max_workgroups) pl.stepper_blocks_cap = std::min(pl.stepper_blocks_cap, s.max_workgroups);
    if (knobs[MAX_BLOCKS])
        pl.stepper_blocks_cap = (uint32_t)std::min<uint64_t>(pl.stepper_blocks_cap, knobs[MAX_BLOCKS]);

    // Replicate rotation (bin store, 256-lane blocks): on when lanes have at least three
    // replicates each (ECDNA_SSA_ROTATE = 0 off, 1 on whenever possible, 2 auto); with two (C4 8-GPU shard)
    // the drain control is faster (74 ms against 84). Auto also leaves it off when the caller gave a cost
    // hint: the costliest-first start order then already balances the lanes, and parking only mixes the
    // order up again (C4 whole sweep, same box: 710-718 ms without rotation against 738-750 with it under
    // the 128-VGPR build, 747-749 against 792-805 under the default one). Results do not depend on it.
    // Byte offsets into bags/park are u32 in the kernel: chunks stay below 2 GiB of either.
    uint64_t rot_mode = knobs[ROTATE];
    // Rotation hands a parked replicate only to lanes of the same partition, partition = XCC id mod
    // kRotParts, and relies on those lanes sharing one L2 (the parked state is read with L1-bypassing
    // loads). That holds when the agent has at most kRotParts XCCs (gfx950 SPX: 8, CPX: 1); otherwise
    // two L2s would share a partition, so rotation stays off.
    if (f.xccs < 1 || f.xccs > (int)kRotParts) rot_mode = 0;
    for (auto& ch : pl.chunks) {
        const uint64_t need = (ch.n + s.stepper_block - 1) / s.stepper_block;
        const uint64_t lanes = std::max<uint64_t>(1, std::min<uint64_t>(need, pl.stepper_blocks_cap)) * s.stepper_block;
        const bool ok = s.bin_k && s.stepper_block == (uint32_t)kStepperBlock &&
                        (uint64_t)ch.n * std::max<uint64_t>(s.bag_bytes, kParkVecs * 16u) < (1ull << 31);
        if (!ok || rot_mode == 0 || (rot_mode == 2 && (ch.n < 3 * lanes || s.hinted))) continue;
        const uint32_t per = (ch.n + kRotParts - 1) / kRotParts;
        ch.rot_n_pad = (per + kRotBlock - 1) / kRotBlock * kRotBlock;
        pl.any_rotation = true;
    }
    if (pl.any_rotation) {
        pl.rot_n_pad_max = (pl.chunk_reps + kRotParts - 1) / kRotParts + kRotBlock;
        // park only while at least 1.5 partition grids' worth of replicates wait; below that the lanes run
        // their replicates to the end (C3 sweep, DESIGN.md §5: 0.5 / 1 / 2 / 3 grids -> 88.2 / 87.2 / 87.1 / 97.5 ms)
        const uint64_t lanes_all = (uint64_t)pl.stepper_blocks_cap * s.stepper_block;
        pl.rot_park_min = (int32_t)(knobs.is_set[ROT_PARK_MIN] ? knobs[ROT_PARK_MIN]
                                                               : std::max<uint64_t>(1, lanes_all * 3 / 2 / kRotParts));
    }

    // grid and drain control per chunk. Drain control (bin store, 256-lane blocks, one wave per SIMD per block):
    // when lanes run more than two replicates each, the youngest wave slot of every SIMD stops taking fresh
    // replicates once fewer than 1.5 grids' worth are left (C3: 105 -> 101 ms). ECDNA_SSA_ADMIT=0:
    // off. Rotation replaces it.
    for (auto& ch : pl.chunks) {
        // (paired lanes: owners only)
        const uint32_t per_block = pl.schedule == 3 ? s.stepper_block / 2 : s.stepper_block;
        const uint32_t need = (ch.n + per_block - 1) / per_block;
        ch.blocks = std::max<uint32_t>(1, std::min<uint32_t>(need, pl.stepper_blocks_cap));
        const uint64_t lanes = (uint64_t)ch.blocks * s.stepper_block;
        const uint32_t per_cu_ch = f.cus ? (uint32_t)((ch.blocks + f.cus - 1) / f.cus) : 0u;
        if (!ch.rot_n_pad && s.bin_k && s.stepper_block == 256 && per_cu_ch >= 2 && ch.n > 2 * lanes && knobs[ADMIT]) {
            const uint32_t slots = (uint32_t)std::min<uint64_t>(knobs[ADMIT_SLOTS], per_cu_ch - 1);
            ch.admit_slot = per_cu_ch - std::max<uint32_t>(slots, 1u);
            ch.admit_remaining = (uint32_t)std::min<uint64_t>(lanes * knobs[ADMIT_X8] / 8, ch.n);
        }
    }
    return pl;
}

}  // namespace plan
}  // namespace ecdna
