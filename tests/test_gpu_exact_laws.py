"""The HIP engine against exact laws (tests/exact_law.py): the GPU steppers compared with mathematics, not with the
oracle. A mistake that csrc/ and oracle/ share passes every parity test; it does not pass these.

Each test runs 2^20 replicates (the one-event pick 2^22, in four launches) of a scenario small enough to enumerate
exactly, and asserts, per scenario: the chi-square of stop reason x final (n-, n+) and of the event count; the four
events_by_type totals, the uneven total, the pooled histogram's k = 0, 1, 2, >= 3 cell counts and the mean final time
against their exact means by z with the exact per-replicate variance; and, where the final rows are downloaded, the
omnibus chi-square over final states. One-event runs pin the channel, the waiting time (KS against Exp(a0)), the
split of one k-copy cell against Binomial(2k, 1/2) at the popcount block edges, the bin K edges and the BINV/BTPE
switch, and the uniform pick (cells of 1, 2 and 70 copies: counters and the large-k row). The time stop is pinned by
the Yule closed form. Every p-value must exceed exact_law.P_MIN = 1e-6; seeds are fixed and the engine is
deterministic, so a test passes or fails forever. tests/test_exact_laws.py makes the same runs on the CPU oracle
(whose outputs the engine's equal bit for bit), so it shows without a GPU whether each seed passes; no seed was
changed.

Variants (VARIANTS below): the row store with the LDS window on and off; the bin store at K = 32, 64 and 256 with
u16/u32 counters as the K implies and with u32 counters forced by cell_cap = 70,000; the instruction schedules
ECDNA_SSA_SCHED 0, 1 and 3; paired lanes; two workgroups, so that lanes refill some 2,000 times; the event hash
off (the bench's TF = 0 instances) and on (TF = 1); the reference-draws stepper. Rows are downloaded for the base
variants of the row store, K = 32, K = 64 and reference draws; K = 256 (whose row download expands 2^20 x 256
counters on the host) and the other variants are checked on summaries, totals and histogram. Variants of one draw
mapping give the same outputs; the statistics are computed once per distinct output (keyed by a digest of it).

Measured on an MI355X: the 445 law tests all passed, 64 s in all; the slowest are the one-event pick in the bin store
(1.3-1.6 s: four launches with rows) and the first joint-state test (0.8 s); the others take 0.1-0.7 s. The lowest
p-value per scenario over all its variants (each equals the oracle's in tests/test_exact_laws.py, whose docstring has
the state counts and enumeration times):
  bd_binomial 0.157 (mean_time, bins32)          pb_binomial 0.0142 (omnibus, bins32)
  pb_no_nminus 0.0156 (mean_time, ref)           bd_no_uneven 0.0473 (cells_k2, ref)
  bd_deterministic 0.00598 (cells_k1, bins32)    bd_extinction 0.0507 (mean_death_nplus, ref)
  bd_cap_compat 0.14 (stop_x_cells, ref)         multi_set 0.0229 (set0/stop_x_cells, ref)
  channel + time 0.0157 (channel, ref)           split 0.0146 (split_hist, k = 64, ref)
  split, no-uneven 0.103 (mean_k1, k = 3, rows)  pick 0.144 (ref)          Yule time stop 0.865 (cells)
Everything in this file ran on the GPU. Not covered: split laws beyond k = 2047 with u32 counters forced by
cell_cap = 70,000 (the engine takes at most 4096 histogram bins and rows of 70,000 cells x 2^20 replicates cannot be
downloaded; K = 32 uses u32 counters at every cell_cap and covers that path with rows).
"""
import hashlib
from dataclasses import dataclass, replace

import numpy as np
import pytest

import exact_law as X
from ecdna_evo_amd import abi

H = abi.FLAG_EVENT_HASH


@dataclass(frozen=True)
class Variant:
    name: str
    store: str
    flags: int = 0
    env: tuple = ()
    kw: tuple = ()
    rows: bool = False


def _variants():
    v = [Variant("rows", "rows", H, rows=True),
         Variant("rows_window0", "rows", H, env=(("ECDNA_SSA_WINDOW", "0"),)),
         Variant("rows_window1", "rows", H, env=(("ECDNA_SSA_WINDOW", "1"),)),
         Variant("rows_nohash", "rows", 0),
         Variant("rows_blocks2", "rows", H, env=(("ECDNA_SSA_MAX_BLOCKS", "2"),))]
    c32 = (("cell_cap", 70_000), ("big_cap", 16))
    for K in (32, 64, 256):
        s = f"bins{K}"
        v += [Variant(s, s, 0, rows=K != 256),
              Variant(f"{s}_hash", s, H),
              Variant(f"{s}_c32", s, 0, kw=c32),
              Variant(f"{s}_c32_hash", s, H, kw=c32),
              Variant(f"{s}_blocks2", s, 0, env=(("ECDNA_SSA_MAX_BLOCKS", "2"),)),
              Variant(f"{s}_pair", s, 0, env=(("ECDNA_SSA_PAIR", "1"),)),
              Variant(f"{s}_pair_blocks2", s, 0, env=(("ECDNA_SSA_PAIR", "1"), ("ECDNA_SSA_MAX_BLOCKS", "2")))]
        v += [Variant(f"{s}_sched{q}", s, 0, env=(("ECDNA_SSA_SCHED", q),)) for q in ("0", "1", "3")]
    v += [Variant("bins64_pair_hash", "bins64", H, env=(("ECDNA_SSA_PAIR", "1"),)),
          Variant("ref", "ref", H, rows=True),
          Variant("ref_nohash", "ref", 0),
          Variant("ref_blocks2", "ref", H, env=(("ECDNA_SSA_MAX_BLOCKS", "2"),))]
    return {x.name: x for x in v}


VARIANTS = _variants()
_MEMO: dict = {}


def run_variant(engine_mod, monkeypatch, spec_of, var: Variant):
    for k, val in var.env:
        monkeypatch.setenv(k, val)
    return engine_mod.run(spec_of(var.store, flags=var.flags, **dict(var.kw)), want_rows=var.rows)


def _digest(res) -> bytes:
    h = hashlib.blake2b(digest_size=16)
    for f in res.summaries.dtype.names:
        if f != "event_hash":  # the only output the hash flag changes
            h.update(np.ascontiguousarray(res.summaries[f]).tobytes())
    h.update(res.hist.tobytes())
    h.update(res.totals.tobytes())
    return h.digest()


def check_once(laws, res, label):
    """exact_law.check_sets, computed once per distinct output. An entry computed with rows carries the omnibus test
    too and serves the row-less variants of the same output."""
    key = (tuple(law.sc.name for law in laws), _digest(res))
    ps = _MEMO.get(key)
    if ps is None or (res.rows is not None and not any(k.endswith("omnibus") for k in ps)):
        ps = _MEMO[key] = X.check_sets(laws, res)
    X.assert_laws(ps, label)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", sorted(X.SCENARIOS))
def test_gpu_joint_state_law(name, variant, engine_mod, monkeypatch):
    sc = X.SCENARIOS[name]
    res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.scenario_spec(sc, store, **kw), VARIANTS[variant])
    check_once([X.enumerate_law(sc)], res, f"{name}/{variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_multi_set_law(variant, engine_mod, monkeypatch):
    """One launch of four parameter sets with their own rates and initial distributions: each set's 2^18 replicates,
    its histogram and its totals record against that set's law."""
    res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.scenario_spec(X.MULTI_SET, store, **kw),
                      VARIANTS[variant])
    check_once([X.enumerate_law(sc) for sc in X.MULTI_SET], res, f"multi_set/{variant}")


ONE_EVENT = ["rows", "rows_nohash", "bins32", "bins32_hash", "bins64", "bins64_hash", "bins64_c32", "bins256",
             "bins256_hash", "ref"]


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("variant", ONE_EVENT)
def test_gpu_one_event_channel_and_time(variant, f32, engine_mod, monkeypatch):
    """The 4-way channel law where all four propensities differ, and the waiting time against Exp(a0) (KS; f64 clock
    and FLAG_TIME_F32)."""
    var = VARIANTS[variant]
    for i in range(len(X.CHANNEL_POPS)):
        res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.channel_spec(i, store, f32, **kw),
                          replace(var, rows=False))
        X.assert_laws(X.check_channel(res, i), f"channel{i}/{variant}/f32={int(f32)}")


@pytest.mark.gpu
@pytest.mark.parametrize("k,variant", [(k, v) for k in X.SPLIT_KS
                                       for v in ("rows", "bins32", "bins64", "bins64_c32", "bins256", "ref")
                                       if X.split_reads_hist(k) or v != "bins64_c32"])  # (no rows at cell_cap 70,000)
def test_gpu_one_event_split(k, variant, engine_mod, monkeypatch):
    """One division of one k-copy cell against Binomial(2k, 1/2): folded, from the device histogram, in every store;
    unfolded (k1 is the first daughter of the final row) in the row store and the reference-draws stepper."""
    var = replace(VARIANTS[variant], rows=X.split_needs_rows(k, VARIANTS[variant].store))
    res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.split_spec(k, store, **kw), var)
    X.assert_laws(X.check_split(res, k, ordered_rows=var.store in ("rows", "ref")), f"split{k}/{variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rows", "bins32", "bins64", "bins256", "ref"])
@pytest.mark.parametrize("k", X.NO_UNEVEN_KS)
def test_gpu_one_event_split_no_uneven(k, variant, engine_mod, monkeypatch):
    """The no-uneven rule at k = 1, 2, 3, where redraws dominate (a draw is rejected with probability 2^(1-2k))."""
    var = replace(VARIANTS[variant], rows=X.split_needs_rows(k, VARIANTS[variant].store))
    res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.split_spec(k, store, no_uneven=True, **kw), var)
    X.assert_laws(X.check_split(res, k, no_uneven=True, ordered_rows=var.store in ("rows", "ref")),
                f"split_no_uneven{k}/{variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rows", "bins32", "bins64", "ref"])
def test_gpu_one_event_pick(variant, engine_mod, monkeypatch):
    """The pick among 3 one-copy, 2 two-copy and 4 seventy-copy cells is 3 : 2 : 4: in the bin store the first five
    sit in counters and the last four in the large-k row, at K = 32 and at K = 64."""
    var = VARIANTS[variant]
    counts = [X.picked_counts(engine_mod.run(spec, want_rows=True))
              for spec in X.pick_specs(var.store, flags=var.flags)]
    X.assert_laws(X.check_pick(counts), f"pick/{variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("variant", ["rows", "bins32", "bins64", "bins256", "bins64_hash", "ref"])
def test_gpu_yule_time_stop(variant, f32, engine_mod, monkeypatch):
    """Pure birth at b0 = b1 = 1 from one cell, stopped by max_time = ln 2: every run stops with MaxTime at the first
    stop test past t, one event after the Yule population N(t): P(final cells = n + 1) = e^-t (1 - e^-t)^(n-1)."""
    var = VARIANTS[variant]
    res = run_variant(engine_mod, monkeypatch, lambda store, **kw: X.yule_spec(store, f32, **kw),
                      replace(var, rows=False))
    X.assert_laws(X.check_yule(res), f"yule/{variant}/f32={int(f32)}")


@pytest.mark.gpu
def test_gpu_variants_launch_the_kernel_instances_they_name(engine_mod, monkeypatch):
    """The variants are different kernels, not one kernel measured again: the instance each context launches
    (ecdna_ssa_ctx_instance) on the birth-death scenario at 2^20 replicates."""
    sc = X.SCENARIOS["bd_binomial"]

    def instance(name):
        var = VARIANTS[name]
        with monkeypatch.context() as m:
            for k, val in var.env:
                m.setenv(k, val)
            with engine_mod.Context(X.scenario_spec(sc, var.store, flags=var.flags, **dict(var.kw))) as ctx:
                ctx.launch()
                ctx.sync()
                return ctx.instance()

    got = {name: instance(name) for name in VARIANTS}
    for name, ins in got.items():
        var = VARIANTS[name]
        assert ins["kernel"] == {"rows": 0, "ref": 2}.get(var.store, 1), name
        if ins["kernel"] == 1:
            assert ins["bin_kmax"] == X.STORES[var.store][1], name
            assert ins["runtime_flags"] == (1 if var.flags & H else 0), name  # TF = 0: the bench's instances
            assert ins["bin_c32"] == (1 if (var.kw or ins["bin_kmax"] == 32) else 0), name
        if "ECDNA_SSA_MAX_BLOCKS" in dict(var.env):
            assert 0 < ins["grid_lanes"] <= 2 * ins["block_lanes"], name
        else:
            assert ins["grid_lanes"] > 2 * ins["block_lanes"], name
    assert got["rows"]["window"] == 1 and got["rows_window1"]["window"] == 1 and got["rows_window0"]["window"] == 0
    # ECDNA_SSA_SCHED: 0 occupancy-first, 1 max-ILP, 3 the 128-VGPR build, which exists at K = 64 with u16 counters
    for K in (32, 64, 256):
        assert got[f"bins{K}_sched0"]["schedule"] == 0 and got[f"bins{K}_sched1"]["schedule"] == 1
        assert got[f"bins{K}_sched3"]["schedule"] == (2 if K == 64 else 0)
    # paired lanes exist for birth-death at K = 32 and 64
    for name in ("bins32_pair", "bins64_pair", "bins64_pair_hash", "bins32_pair_blocks2", "bins64_pair_blocks2"):
        assert got[name]["paired"] == 1 and got[name]["schedule"] == 3, name
    assert got["bins256_pair"]["paired"] == 0 and got["bins64"]["paired"] == 0
