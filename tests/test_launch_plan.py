"""The launch planner of ecdna_ssa_ctx_create on the CPU (ecdna-evo_amd/csrc/ssa_plan.hpp): chunk size, the bin
stepper's schedule and grid, replicate rotation and the drain control are one pure function of the run's shape, the
device's facts and the ECDNA_SSA_* knobs, so every decision, the per-chunk values no ecdna_ssa_instance_t field shows
included (rot_n_pad, rot_park_min, admit_slot, admit_remaining), is checked here without a GPU.

tests/native/plan_check.cpp is built for the host alone with the address and undefined-behaviour sanitizers and prints
the plan of each case it reads. The bench shapes are bench.workload_spec's own; the facts are stated inputs, not
measurements: 256 CUs, 8 XCCs, 256 GiB free, the occupancies of tests/test_instance_rules.py's table (and 4 workgroups
per CU for the 128-VGPR build). Every expected value below is worked out from the rules by hand, in the comment beside
it; tests/test_gpu_bench_instances.py asserts the same instances on hardware."""
import pytest

import bench
from ecdna_evo_amd import abi, shard
from support import native

GIB = 1 << 30
OFF = 0xFFFFFFFF  # admit_slot of a chunk without the drain control
FACTS = dict(cus=256, xccs=8, free=256 * GIB)
# workgroups per CU of the bin stepper's builds: 0 default, 1 max-ILP, 2 the 128-VGPR build, 3 paired lanes (0: no such
# instance; the paired builds' figures only have to be >= 1, see test_c5_shard_pairs_at_any_pair_occupancy)
OCC_K32 = dict(occ0=4, occ1=4, occ3=2)  # K = 32 / u32: LDS bounds both builds at 4
OCC_K32_PURE_BIRTH = dict(occ0=4, occ1=4)  # no paired instance
OCC_K64_U32 = dict(occ0=2, occ1=2, occ3=2)  # LDS bounds both builds at 2
OCC_K64_U16 = dict(occ0=4, occ1=3, occ2=4, occ3=2)


pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = native.build(tmp_path_factory, "plan_check")

    def run(cases):
        """cases: dicts of plan_check's words. Returns per case (plan fields, [chunk fields]), all integers but
        rot_parts (a list of them)."""
        text = "".join(" ".join(f"{k}={v}" for k, v in c.items()) + "\n" for c in cases)
        res = []
        for line in native.run(exe, stdin=text):
            kind, *words = line.split()
            d = dict(w.split("=") for w in words)
            d = {k: [int(x) for x in v.split(",")] if k == "rot_parts" else int(v) for k, v in d.items()}
            if kind == "plan":
                res.append((d, []))
            else:
                res[-1][1].append(d)
        assert len(res) == len(cases)
        return res

    return run


def shape_of(spec, snap_stats=0, passages=0, passage_cells=0, block=256):
    """plan_check's words for a RunSpec: the scalar parameters the planner reads, from the ABI struct itself."""
    p = spec.params()
    return dict(n=p.n_replicates, process=p.process, flags=p.flags, cell_cap=p.cell_cap, big_cap=p.big_cap,
                bin_kmax=p.bin_kmax, n_snapshots=p.n_snapshots, max_workgroups=p.max_workgroups,
                hinted=int(bool(p.set_cost_hint)), snap_stats=snap_stats, passages=passages,
                passage_cells=passage_cells, block=block)


def bench_case(workload, n=None, world=1, rank=0, occ=None, **extra):
    total = bench.WORKLOADS[workload][0]
    if world == 1:
        spec = bench.workload_spec(0, n or total, n or total, workload=workload)
    elif workload == "c3":  # the fixed-total reading: contiguous shards of 2^20
        first, n = shard.shard_range(rank, world, total)
        spec = bench.workload_spec(first, n, total, workload=workload)
    else:
        first, n, stride = shard.interleaved_range(rank, world, total)
        spec = bench.workload_spec(first, n, total, workload=workload, stride=stride)
    return {**shape_of(spec), **FACTS, **occ, **extra}


def one_chunk(res):
    plan, chunks = res
    assert plan["fits"] == 1 and plan["n_chunks"] == 1 and len(chunks) == 1, plan
    assert chunks[0]["first"] == 0 and chunks[0]["n"] == plan["chunk_reps"]
    return plan, chunks[0]


# ------------------------------------------------------------------------------------------------ the bench shapes
#
# The rules, with c = 256 CUs and 256-lane blocks (ssa_plan.hpp; n = the one chunk's replicates):
#   schedule: 3 if birth-death, no snapshots, a paired instance and n <= c * 128 = 32,768; else 1 if n <= c * 256 =
#     65,536; else 2 if K = 64 / u16 without runtime flags and n >= 4 * c * 4 * 256 = 1,048,576; else 1 if
#     occ1 >= occ0 or n < 4 * occ0 * c * 256; else 0.
#   cap = occ[schedule] * c workgroups; blocks = min(ceil(n / 256), cap), under pairs min(ceil(n / 128), cap).
#   rotation (auto): no cost hint and n >= 3 * lanes, lanes = 256 * min(ceil(n / 256), cap); then rot_n_pad =
#     ceil(ceil(n / 8) / 16) * 16 and rot_park_min = cap * 256 * 3 / 2 / 8.
#   drain control: no rotation, ceil(blocks / c) = per_cu >= 2 and n > 2 * blocks * 256; then admit_slot = per_cu - 1
#     and admit_remaining = min(blocks * 256 * 12 / 8, n).
# All fit one chunk of the 0.85 * 256 GiB = 233.6e9 B budget: C3 and C4 hold 10,048 * 2 + K * (4 or 2) + 68 = 20,292 B
# per replicate (4,194,304 of them: 85.1e9 B), C5 65,536 * 2 + 256 + 68 = 131,396 B (262,144: 34.4e9 B).


def test_c3_rotates(plans):
    """C3, 2^20 replicates, K = 32 / u32: n > 65,536 and occ1 = occ0 = 4: schedule 1, cap 4 * 256 = 1,024 = blocks
    (ceil(n / 256) = 4,096), lanes 262,144; n = 4 lanes >= 3 lanes: rotation, rot_n_pad = 2^20 / 8 = 131,072 (a
    multiple of 16), every partition starts with 131,072 waiting and fresh, rot_park_min = 262,144 * 3 / 2 / 8 =
    49,152; rotation replaces the drain control."""
    plan, ch = one_chunk(plans([bench_case("c3", occ=OCC_K32)])[0])
    assert (plan["bin_k"], plan["bin_c32"], plan["rep_bytes"]) == (32, 1, 20_292)
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"], plan["stepper_block"]) == (1, 1024, 1024, 256)
    assert (plan["any_rotation"], ch["rot_n_pad"], plan["rot_park_min"]) == (1, 131_072, 49_152)
    assert ch["rot_parts"] == [131_072] * 8 and plan["rot_n_pad_max"] == 131_072 + 16 and plan["rot_tick_log2"] == 10
    assert (ch["admit_slot"], ch["admit_remaining"]) == (OFF, 0)


def test_c3_fixed_total_shard(plans):
    """C3's 8-GPU shard of a fixed 2^20, 131,072 replicates: schedule 1 as above, cap 1,024, blocks = ceil(n / 256) = 512
    (2 per CU), lanes 131,072 = n: no rotation (n < 3 lanes), no drain control (n is not > 2 lanes)."""
    plan, ch = one_chunk(plans([bench_case("c3", world=8, rank=7, occ=OCC_K32)])[0])
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"]) == (1, 1024, 512)
    assert (plan["any_rotation"], ch["rot_n_pad"], ch["admit_slot"], ch["admit_remaining"]) == (0, 0, OFF, 0)


def test_c4_whole_sweep_drains(plans):
    """C4 on one GPU, 4,194,304 replicates, K = 64 / u16, cost hint: n >= 1,048,576 without runtime flags: schedule 2,
    cap occ2 * 256 = 1,024 = blocks, lanes 262,144; hinted: no rotation; per_cu 4 and n > 524,288: drain control,
    admit_slot = 4 - max(min(1, 3), 1) = 3, admit_remaining = min(262,144 * 12 / 8, n) = 393,216."""
    plan, ch = one_chunk(plans([bench_case("c4", occ=OCC_K64_U16)])[0])
    assert (plan["bin_k"], plan["bin_c32"], plan["rep_bytes"]) == (64, 0, 20_292)
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"]) == (2, 1024, 1024)
    assert (plan["any_rotation"], ch["rot_n_pad"], ch["admit_slot"], ch["admit_remaining"]) == (0, 0, 3, 393_216)


@pytest.mark.parametrize("pair_occ", [1, 2, 4])
def test_c5_shard_pairs_at_any_pair_occupancy(plans, pair_occ):
    """C5's 8-GPU shard, 32,768 replicates, K = 64 / u32: birth-death, no snapshots, n <= 32,768: schedule 3; a paired
    block runs 128 replicates: blocks = min(ceil(n / 128), cap) = 256 (1 per CU) for any cap = pair_occ * 256 >= 256,
    65,536 lanes; rotation's lanes divide by 256: 128 blocks, n < 3 * 32,768: off; per_cu 1: no drain control."""
    plan, ch = one_chunk(plans([bench_case("c5", world=8, occ={**OCC_K64_U32, "occ3": pair_occ})])[0])
    assert (plan["bin_k"], plan["bin_c32"], plan["rep_bytes"]) == (64, 1, 131_396)
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"]) == (3, pair_occ * 256, 256)
    assert (plan["any_rotation"], ch["rot_n_pad"], ch["admit_slot"], ch["admit_remaining"]) == (0, 0, OFF, 0)


def test_c2_c5_whole_and_c4_shard(plans):
    """C2, 65,536 replicates of pure birth (no paired instance), K = 32: n <= 65,536: schedule 1, cap 1,024, blocks 256
    (1 per CU): neither rotation (n = lanes) nor the drain control.
    C5 on one GPU, 262,144, K = 64 / u32 (occ 2 / 2): n > 65,536, occ1 >= occ0: schedule 1, cap 512 = blocks, lanes
    131,072: n = 2 lanes: no rotation (< 3 lanes), no drain control (not > 2 lanes).
    C4's 8-GPU shard, 524,288, K = 64 / u16 (occ 4 / 3), hinted: n < 1,048,576 = 4 * occ0 * c * 256: schedule 1, cap
    3 * 256 = 768 = blocks, lanes 196,608; no rotation (hinted; and n < 589,824); per_cu 3, n > 393,216: drain control,
    admit_slot 3 - 1 = 2, admit_remaining = min(196,608 * 12 / 8, n) = 294,912."""
    c2, c5, c4 = plans([bench_case("c2", occ=OCC_K32_PURE_BIRTH), bench_case("c5", occ=OCC_K64_U32),
                        bench_case("c4", world=8, rank=3, occ=OCC_K64_U16)])
    plan, ch = one_chunk(c2)
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"], ch["rot_n_pad"], ch["admit_slot"]) == (1, 1024, 256, 0, OFF)
    plan, ch = one_chunk(c5)
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"], ch["rot_n_pad"], ch["admit_slot"]) == (1, 512, 512, 0, OFF)
    plan, ch = one_chunk(c4)
    assert ch["n"] == 524_288
    assert (plan["schedule"], plan["blocks_cap"], ch["blocks"], ch["rot_n_pad"]) == (1, 768, 768, 0)
    assert (ch["admit_slot"], ch["admit_remaining"]) == (2, 294_912)


# ------------------------------------------------------------------------------------------------ chunking
#
# A row-store run of cell_cap 100: rows of round_up(100, 64) = 128 u16 cells, 256 B per replicate and nothing else.

def rows_case(n, **extra):
    spec = abi.RunSpec(seed=1, process=abi.BIRTH_DEATH, rates=((1.0, 1.5, 0.3, 0.3),), n_replicates=n, max_cells=100)
    return {**shape_of(spec), **FACTS, "occ_rows": 8, **extra}


def test_chunking_edges(plans):
    res = plans([
        rows_case(0),                                  # no replicates: buffers for one, no chunk
        rows_case(20, ECDNA_SSA_MAX_CHUNK=7),          # 7 + 7 + 6
        rows_case(20, ECDNA_SSA_MAX_ROW_BYTES=255),    # less than one replicate: the error
        rows_case(3, ECDNA_SSA_MAX_ROW_BYTES=256),     # exactly one replicate per chunk
        rows_case(3, ECDNA_SSA_MAX_ROW_BYTES=511),     # (and still one)
        rows_case(3, free=301),                        # (uint64)(301 * 0.85) = 255 B: the error
        rows_case(3, free=302),                        # (uint64)(302 * 0.85) = 256 B: one
        rows_case(3, free=302, ECDNA_SSA_MAX_ROW_BYTES=10_000),  # the knob only lowers the budget
        rows_case(20, ECDNA_SSA_MAX_ROW_BYTES=256 * 9, ECDNA_SSA_MAX_CHUNK=12),  # fit 9, then capped by 12: 9
    ])
    assert res[0][0]["rep_bytes"] == 256 and res[0][0]["row_stride"] == 128
    assert (res[0][0]["fits"], res[0][0]["chunk_reps"], res[0][1]) == (1, 1, [])
    assert res[1][0]["chunk_reps"] == 7 and [(c["first"], c["n"], c["blocks"]) for c in res[1][1]] == \
        [(0, 7, 1), (7, 7, 1), (14, 6, 1)]
    assert (res[2][0]["fits"], res[2][0]["chunk_reps"], res[2][1]) == (0, 0, [])
    for r in (res[3], res[4], res[6], res[7]):
        assert r[0]["chunk_reps"] == 1 and [(c["first"], c["n"]) for c in r[1]] == [(0, 1), (1, 1), (2, 1)]
    assert res[5][0]["fits"] == 0
    assert res[8][0]["chunk_reps"] == 9 and [c["n"] for c in res[8][1]] == [9, 9, 2]


def test_per_replicate_bytes(plans):
    """What a replicate of a chunk holds besides its 256 B row: snapshot rows where they are chunk scratch (snapshot
    statistics without the run's rows: 2 snapshots x 128 cells x 2 B = 512 B; the run's rows exist only under
    ECDNA_FLAG_SNAPSHOT_ROWS = 0x8 with n > 0), founders in a passage run (round_up(100, 64) = 128 cells x 2 B + the 8 B
    of {n-, n+}); in the bin store its counters and 68 B of parked state (K = 64: u16 counters up to cell_cap 65,535)."""
    stats = abi.FLAG_REP_STATS
    res = plans([
        rows_case(5, flags=stats, n_snapshots=2, snap_stats=1),
        rows_case(5, flags=stats | 0x8, n_snapshots=2, snap_stats=1),
        rows_case(0, flags=stats | 0x8, n_snapshots=2, snap_stats=1),
        rows_case(5, flags=stats | 0x8, n_snapshots=2),
        rows_case(5, flags=stats, passages=3, passage_cells=100),
        rows_case(5, flags=abi.FLAG_BIN_STORE, bin_kmax=64, cell_cap=65_535, big_cap=100),
        rows_case(5, flags=abi.FLAG_BIN_STORE, bin_kmax=64, cell_cap=65_536, big_cap=100),
        rows_case(5, flags=abi.FLAG_BIN_STORE, bin_kmax=64, cell_cap=65_535, big_cap=100, ECDNA_SSA_C32=1),
        rows_case(5, flags=abi.FLAG_BIN_STORE, bin_kmax=0, cell_cap=200, big_cap=0),
    ])
    assert [(r[0]["snap_rows_local"], r[0]["rep_bytes"]) for r in res[:5]] == \
        [(1, 768), (0, 256), (1, 768), (0, 256), (0, 256 + 256 + 8)]
    # large-k rows of big_cap 100 -> 128 cells = 256 B; K = 64 counters 128 B (u16) or 256 B (u32); 68 B parked
    assert [(r[0]["bin_k"], r[0]["bin_c32"], r[0]["rep_bytes"]) for r in res[5:8]] == \
        [(64, 0, 256 + 128 + 68), (64, 1, 256 + 256 + 68), (64, 1, 256 + 256 + 68)]
    # bin_kmax 0 = 64; big_cap 0 = cell_cap 200 -> 256 cells = 512 B
    assert (res[8][0]["bin_k"], res[8][0]["row_stride"], res[8][0]["rep_bytes"]) == (64, 256, 512 + 128 + 68)


# ------------------------------------------------------------------------------------------------ the knobs, once each

def test_grid_knobs(plans):
    """Row store, 10^6 replicates: the occupancy (8) is capped at 3 workgroups per CU, 768 blocks; BLOCKS_PER_CU
    overrides the cap; then the floor of 1, then max_workgroups, then MAX_BLOCKS."""
    res = plans([
        rows_case(10**6),
        rows_case(10**6, occ_rows=2),
        rows_case(10**6, ECDNA_SSA_BLOCKS_PER_CU=5),
        rows_case(10**6, occ_rows=0),
        rows_case(10**6, max_workgroups=100),
        rows_case(10**6, ECDNA_SSA_MAX_BLOCKS=1),
        rows_case(10**6, ECDNA_SSA_BLOCKS_PER_CU=5, max_workgroups=2000, ECDNA_SSA_MAX_BLOCKS=1000),
        rows_case(10**6, ECDNA_SSA_WINDOW=0, ECDNA_SSA_ROT_TICK=40),
        rows_case(10**6, ECDNA_SSA_WINDOW=5, ECDNA_SSA_ROT_TICK=11),
        rows_case(1000),
    ])
    caps = [one_chunk(r) for r in res]
    assert [(p["blocks_cap"], c["blocks"]) for p, c in caps[:7]] == \
        [(768, 768), (512, 512), (1280, 1280), (256, 256), (100, 100), (1, 1), (1000, 1000)]
    assert [(p["window"], p["rot_tick_log2"]) for p, _ in caps[6:9]] == [(1, 10), (0, 30), (1, 11)]
    assert caps[9][1]["blocks"] == 4  # ceil(1000 / 256)
    for p, c in caps:  # the row store has neither rotation nor the drain control
        assert (p["schedule"], p["any_rotation"], c["rot_n_pad"], c["admit_slot"]) == (0, 0, 0, OFF)


def test_reference_draws_take_their_own_occupancy_and_block(plans):
    """ECDNA_FLAG_REFERENCE_DRAWS (0x40; row store): the reference-draws stepper's occupancy, uncapped, at its own
    workgroup size: 5 * 256 = 1,280 blocks of 64 lanes for 10^6 replicates."""
    plan, ch = one_chunk(plans([rows_case(10**6, flags=0x40, occ_ref=5, block=64)])[0])
    assert (plan["blocks_cap"], ch["blocks"], plan["stepper_block"], ch["admit_slot"]) == (1280, 1280, 64, OFF)


def test_schedule_and_pair_knobs(plans):
    """C3 with occ 4 / 3: SCHED = 0 keeps the default build (cap 1,024), SCHED = 1 takes max-ILP (cap 768). The C5 shard
    with PAIR = 0: n <= 65,536: schedule 1, cap 512, blocks ceil(32,768 / 256) = 128. C5 whole with PAIR = 1: schedule
    3, cap occ3 * 256 = 512 = blocks (ceil(262,144 / 128) = 2,048), lanes 131,072: neither rotation nor drain control.
    C4 whole with C32 = 1 is K = 64 / u32: not the 128-VGPR build; occ1 < occ0 and n >= 1,048,576: schedule 0."""
    occ = dict(occ0=4, occ1=3, occ3=2)
    res = plans([
        bench_case("c3", occ=occ, ECDNA_SSA_SCHED=0), bench_case("c3", occ=occ, ECDNA_SSA_SCHED=1),
        bench_case("c5", world=8, occ=OCC_K64_U32, ECDNA_SSA_PAIR=0),
        bench_case("c5", occ=OCC_K64_U32, ECDNA_SSA_PAIR=1),
        bench_case("c4", occ=OCC_K64_U16, ECDNA_SSA_C32=1),
        bench_case("c4", occ=OCC_K64_U16, ECDNA_SSA_SCHED=3),
    ])
    got = [one_chunk(r) for r in res]
    assert [(p["schedule"], p["blocks_cap"], c["blocks"]) for p, c in got] == \
        [(0, 1024, 1024), (1, 768, 768), (1, 512, 128), (3, 512, 512), (0, 1024, 1024), (2, 1024, 1024)]
    assert (got[3][1]["rot_n_pad"], got[3][1]["admit_slot"]) == (0, OFF)
    assert (got[4][0]["bin_c32"], got[4][0]["rep_bytes"]) == (1, 20_096 + 256 + 68)


def test_rotation_knobs(plans):
    """ROTATE = 1 on the C3 shard (auto leaves it off): rot_n_pad = 131,072 / 8 = 16,384, rot_park_min from the cap's
    lanes, 1,024 * 256 * 3 / 2 / 8 = 49,152, buffers for n_pad_max = ceil(chunk_reps / 8) + 16. ROTATE = 0 on C3 turns it
    off, and the drain control takes over (per_cu 4, n > 524,288: slot 3, 393,216 remaining). ROT_PARK_MIN set to 0 stays
    0 (7 stays 7); an empty value is unset, as in the environment. ROTATE = 1 overrides the cost hint (C4 whole:
    rot_n_pad 524,288)."""
    res = plans([
        bench_case("c3", world=8, occ=OCC_K32, ECDNA_SSA_ROTATE=1),
        bench_case("c3", occ=OCC_K32, ECDNA_SSA_ROTATE=0),
        bench_case("c3", occ=OCC_K32, ECDNA_SSA_ROT_PARK_MIN=0),
        bench_case("c3", occ=OCC_K32, ECDNA_SSA_ROT_PARK_MIN=7),
        bench_case("c3", occ=OCC_K32, ECDNA_SSA_ROT_PARK_MIN="", ECDNA_SSA_ROTATE=""),
        bench_case("c4", occ=OCC_K64_U16, ECDNA_SSA_ROTATE=1),
    ])
    got = [one_chunk(r) for r in res]
    p, c = got[0]
    assert (p["any_rotation"], c["rot_n_pad"], p["rot_park_min"], p["rot_n_pad_max"]) == (1, 16_384, 49_152, 16_400)
    assert c["rot_parts"] == [16_384] * 8 and c["admit_slot"] == OFF
    p, c = got[1]
    assert (p["any_rotation"], c["rot_n_pad"], p["rot_park_min"], p["rot_n_pad_max"]) == (0, 0, 0, 0)
    assert (c["admit_slot"], c["admit_remaining"]) == (3, 393_216)
    assert [(p["any_rotation"], p["rot_park_min"]) for p, _ in got[2:5]] == [(1, 0), (1, 7), (1, 49_152)]
    assert (got[5][1]["rot_n_pad"], got[5][1]["admit_slot"]) == (524_288, OFF)


def test_rotation_needs_known_xccs_within_the_partitions(plans):
    """An XCC count of 0 (the query failed) or above kRotParts = 8 turns rotation off, forced or not; 1 (CPX) keeps it."""
    res = plans([bench_case("c3", occ=OCC_K32, xccs=x, **kn)
                 for x in (0, 16, 9) for kn in ({}, {"ECDNA_SSA_ROTATE": 1})] + [bench_case("c3", occ=OCC_K32, xccs=1)])
    for r in res[:-1]:
        p, c = one_chunk(r)
        assert (p["any_rotation"], c["rot_n_pad"], c["admit_slot"], c["admit_remaining"]) == (0, 0, 3, 393_216)
    assert one_chunk(res[-1])[1]["rot_n_pad"] == 131_072


def test_rotation_offsets_stay_below_2_gib(plans):
    """The kernel's u32 byte offsets: n * max(counter bytes, 64) < 2^31. K = 64 / u32 (cell_cap > 65,535) has 256 B of
    counters: 8,388,607 replicates rotate (rot_n_pad = ceil(ceil(n / 8) / 16) * 16 = 1,048,576; partition 7 holds one
    replicate less), 8,388,608 do not. (452 B per replicate with a 64-cell large-k row: one chunk.)"""
    spec = abi.RunSpec(seed=1, process=abi.BIRTH_DEATH, rates=((1.0, 1.5, 0.3, 0.3),), n_replicates=1, max_cells=100,
                       flags=abi.FLAG_BIN_STORE, bin_kmax=64, cell_cap=70_000, big_cap=64)
    base = {**shape_of(spec), **FACTS, **OCC_K64_U32, "ECDNA_SSA_ROTATE": 1}
    below, at = plans([{**base, "n": (1 << 23) - 1}, {**base, "n": 1 << 23}])
    p, c = one_chunk(below)
    assert p["rep_bytes"] == 452 and (c["rot_n_pad"], c["rot_parts"]) == (1 << 20, [1 << 20] * 7 + [(1 << 20) - 1])
    p, c = one_chunk(at)
    assert (p["any_rotation"], c["rot_n_pad"]) == (0, 0)


def test_drain_control_knobs(plans):
    """C4 whole (per_cu 4, lanes 262,144): ADMIT = 0 turns it off; ADMIT_SLOTS closes min(slots, per_cu - 1) slots, at
    least one: 0 -> slot 3, 2 -> slot 2, 9 -> slot 1; ADMIT_X8 = 8: one grid's worth, 262,144, remaining; = 200: n."""
    res = plans([bench_case("c4", occ=OCC_K64_U16, **kn) for kn in (
        {"ECDNA_SSA_ADMIT": 0}, {"ECDNA_SSA_ADMIT_SLOTS": 0}, {"ECDNA_SSA_ADMIT_SLOTS": 2}, {"ECDNA_SSA_ADMIT_SLOTS": 9},
        {"ECDNA_SSA_ADMIT_X8": 8}, {"ECDNA_SSA_ADMIT_X8": 200})])
    got = [one_chunk(r)[1] for r in res]
    assert [(c["admit_slot"], c["admit_remaining"]) for c in got] == \
        [(OFF, 0), (3, 393_216), (2, 393_216), (1, 393_216), (3, 262_144), (3, 4_194_304)]


# ------------------------------------------------------------------------------------------------ invariants

def _store_case(store, n, **extra):
    flags, kmax, block, occ = {"rows": (0, 0, 256, {"occ_rows": 8}),
                               "k64": (abi.FLAG_BIN_STORE, 64, 256, OCC_K64_U16),
                               "k256": (abi.FLAG_BIN_STORE, 256, 64, dict(occ0=8, occ1=8))}[store]
    spec = abi.RunSpec(seed=1, process=abi.BIRTH_DEATH, rates=((1.0, 1.5, 0.3, 0.3),), n_replicates=n,
                       max_cells=10_000, flags=flags, bin_kmax=kmax)
    return {**shape_of(spec, block=block), **FACTS, **occ, **extra}


# (500,000: between two and three replicates per lane of the K = 64 / u16 max-ILP grid, 196,608 lanes: drain control)
GRID_N = [1, 2, 255, 256, 257, 32_768, 32_769, 65_536, 65_537, 1 << 17, (1 << 18) + 1, 500_000, 786_431, 786_432,
          1 << 20, (1 << 22) + 5, 1 << 24]


@pytest.mark.parametrize("store", ["rows", "k64", "k256"])
def test_plan_invariants_over_a_grid_of_runs(plans, store):
    """n from 1 to 2^24 (the largest rows runs chunk by the budget alone), also in chunks of at most 100,000 and with
    rotation forced: the chunks tile [0, n); 1 <= blocks <= cap; no chunk has both rotation and the drain control;
    rot_n_pad is a multiple of kRotBlock = 16 with kRotParts * rot_n_pad >= the chunk's n, and the partitions' counters
    add up to it."""
    knobs = ({}, {"ECDNA_SSA_MAX_CHUNK": 100_000}, {"ECDNA_SSA_ROTATE": 1}, {"ECDNA_SSA_ROTATE": 1, "ECDNA_SSA_PAIR": 1})
    cases = [_store_case(store, n, **kn) for n in GRID_N for kn in knobs]
    rotated = drained = 0
    for case, (plan, chunks) in zip(cases, plans(cases)):
        n = case["n"]
        assert plan["fits"] == 1 and plan["n_chunks"] == len(chunks) == -(-n // plan["chunk_reps"]), (case, plan)
        at = 0
        for ch in chunks:
            assert ch["first"] == at and 1 <= ch["n"] <= plan["chunk_reps"], (case, ch)
            at += ch["n"]
            assert 1 <= ch["blocks"] <= plan["blocks_cap"], (case, ch)
            assert not (ch["rot_n_pad"] and ch["admit_slot"] != OFF), (case, ch)
            if ch["rot_n_pad"]:
                assert ch["rot_n_pad"] % 16 == 0 and 8 * ch["rot_n_pad"] >= ch["n"], (case, ch)
                assert ch["rot_n_pad"] <= plan["rot_n_pad_max"] and sum(ch["rot_parts"]) == ch["n"], (case, ch)
                assert plan["any_rotation"] == 1
            rotated += bool(ch["rot_n_pad"])
            drained += ch["admit_slot"] != OFF
        assert at == n
        assert plan["any_rotation"] == int(any(ch["rot_n_pad"] for ch in chunks))
    # rotation and the drain control are the 256-lane bin store's alone (and both occur there)
    assert (rotated > 0, drained > 0) == ((True, True) if store == "k64" else (False, False))
