"""Serial passaging on the GPU (ecdna_ssa_passages_t, passage mapping v1; include/ecdna_ssa.h): every
replicate regrown from its own sample, G growth phases in one launch.

The expected results are built from the CPU oracle and the numpy restatements only: phase 0 is oracle.run of the plain
spec; the founders are tests/passage_law.py's; phase g >= 1 is oracle.run under seed_g with one parameter set per
replicate (reps_per_set = 1, the rates repeated) whose initial histogram is that replicate's founders. Summaries (time
bits and event hash included), histograms and totals must match bit for bit; statistics and sample statistics at the
ABC-statistics tolerance of tests/test_gpu_abc_stats.py (1e-12 relative: sums are reduced in a different order on the
GPU; log is ocml's vs numpy's).

A run whose founders hold more cells above bin_kmax than big_cap cannot be built through the ABI: the founders are a
subset of the phase's final population, and the bin store never lets a population hold more than big_cap cells above
bin_kmax (a division that would is refused with ECDNA_REP_ERR_CELL_CAP and leaves the state as it was). The start
loop's guard is therefore a defence the engine cannot be driven into, and no case here reaches it; the
case "bins32-large-k-cell-cap" instead runs K = 32 from {1: 5, 40: 3} with a big_cap so small that replicates stop with
ECDNA_REP_ERR_CELL_CAP in the middle of a phase, and checks that their populations are sampled and carried on exactly
as the oracle chain says.
"""
import numpy as np
import pytest

import passage_law as pl
import subsample_law as sl
from ecdna_evo_amd import abi
from exact_law import MIN_EXPECTED, Scenario, chi2_lumped, enumerate_law
from support.passage_specs import (BD_RATES, BINS, CASES, G, MAX_CELLS, N, PB_RATES, _base, _chain, _passage_spec,
                                   _targets)

RTOL, ATOL = 1e-12, 1e-14
FLOATS = ("mean", "entropy", "frequency", "ks", "mean_rel", "entropy_rel", "frequency_diff")


def _check_stats(got, want, tag):
    assert len(got) == len(want)
    for i in range(len(want)):
        assert int(got[i]["cells"]) == want[i]["cells"], f"{tag} replicate {i}: cells"
        for f in FLOATS:
            np.testing.assert_allclose(got[i][f], want[i][f], rtol=RTOL, atol=ATOL, err_msg=f"{tag} replicate {i}: {f}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_chain(engine_mod, oracle_mod, case):
    name, store, kmax, process, seg, rates, m, extra = case
    base = _base(store, kmax, process, seg, rates, **extra)
    want = _chain(oracle_mod, name, base, m)
    g = engine_mod.run(_passage_spec(base, m), want_rows=True)
    ps = g.passages
    assert ps.summaries.shape == (G, N) and ps.hist.shape == (G, 2, BINS) and ps.totals.shape == (G, 2)
    for ph in range(G):
        w = want[ph]
        for f in abi.SUMMARY_DTYPE.names:
            a, b = ps.summaries[ph][f], w["summaries"][f]
            if f == "time":
                a, b = a.view(np.uint64), b.view(np.uint64)
            np.testing.assert_array_equal(a, b, err_msg=f"{name} phase {ph}: summaries.{f}")
        np.testing.assert_array_equal(ps.hist[ph], w["hist"], err_msg=f"{name} phase {ph}: hist")
        assert ps.totals[ph].tobytes() == w["totals"].tobytes(), f"{name} phase {ph}: totals"
        _check_stats(ps.stats[ph], w["stats"], f"{name} phase {ph} stats")
        _check_stats(ps.sample_stats[ph], w["sample_stats"], f"{name} phase {ph} sample stats")
        np.testing.assert_array_equal(ps.sample_hist[ph], w["sample_hist"], err_msg=f"{name} phase {ph}: sample hist")
    # the ordinary downloads are the last phase's, rows included (one chunk)
    last = G - 1
    assert g.summaries.tobytes() == ps.summaries[last].tobytes() and g.totals.tobytes() == ps.totals[last].tobytes()
    assert g.stats.tobytes() == ps.stats[last].tobytes() and g.sample_stats.tobytes() == ps.sample_stats[last].tobytes()
    np.testing.assert_array_equal(g.hist, ps.hist[last])
    np.testing.assert_array_equal(g.sample_hist, ps.sample_hist[last])
    for i in range(N):
        np.testing.assert_array_equal(g.row(i), want[last]["rows"][i], err_msg=f"{name}: last phase row {i}")
    # what the case is about
    s = ps.summaries
    cells = s["nminus"] + s["nplus"]
    if m == 4096:  # the whole population is carried: the next phase stops at MaxCells before its first event
        full = cells[0] >= MAX_CELLS
        assert full.any() and np.all(s["iters"][1][full] == 0) and np.all(s["stop_reason"][1][full] == abi.STOP_MAX_CELLS)
        np.testing.assert_array_equal(cells[1][full], cells[0][full])
    if "extinctions" in name:
        dead = cells[0] == 0
        assert dead.any() and not dead.all()
        assert np.all(s["error"][1][dead] == abi.REP_ERR_EMPTY) and np.all(s["stop_reason"][1][dead] == abi.STOP_ERROR)
        assert np.all(s["iters"][1][dead] == 0)
    if "large-k" in name:
        big = [sum(v for k, v in f.items() if k > kmax) for f in want[0]["founders"]]
        assert max(big) >= 5  # founders above bin_kmax start in the large-k row
    if "cell-cap" in name:
        capped = s["error"] == abi.REP_ERR_CELL_CAP
        assert capped[0].any() and capped[1].any() and (cells[capped] > 0).all()
        assert (s["iters"][1:][capped[:-1]] > 0).any()  # their populations found phases that run


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 64)])
def test_limits(engine_mod, oracle_mod, store, kmax):
    """The pass at its LDS limit: the largest table and founder sort (m' = 4096 of 8,200 cells, 4,096 sort slots) beside
    the largest histogram (2,048 bins), one wave per workgroup. Phase 0 samples by picks; phase 1 starts from 4,096
    founders. The same oracle chain as test_oracle_chain, two phases of 64 replicates."""
    n, phases, max_cells, bins, m = 64, 2, 8200, 2048, 4096
    base = _base(store, kmax, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES, n_replicates=n, reps_per_set=n // 2,
                 max_cells=max_cells, hist_bins=bins, cell_cap=None)
    want = _chain(oracle_mod, f"limits-{store}", base, m, N=n, G=phases, MAX_CELLS=max_cells, BINS=bins)
    ps = engine_mod.run(_passage_spec(base, m, G=phases), want_rows=True).passages
    assert ps.summaries.shape == (phases, n) and ps.sample_hist.shape == (phases, 2, bins)
    assert np.all(ps.summaries[0]["nminus"] + ps.summaries[0]["nplus"] == max_cells)
    for ph in range(phases):
        w = want[ph]
        for f in abi.SUMMARY_DTYPE.names:
            a, b = ps.summaries[ph][f], w["summaries"][f]
            if f == "time":
                a, b = a.view(np.uint64), b.view(np.uint64)
            np.testing.assert_array_equal(a, b, err_msg=f"{store} phase {ph}: summaries.{f}")
        np.testing.assert_array_equal(ps.hist[ph], w["hist"], err_msg=f"{store} phase {ph}: hist")
        assert ps.totals[ph].tobytes() == w["totals"].tobytes(), f"{store} phase {ph}: totals"
        _check_stats(ps.stats[ph], w["stats"], f"{store} phase {ph} stats")
        _check_stats(ps.sample_stats[ph], w["sample_stats"], f"{store} phase {ph} sample stats")
        assert np.all(ps.sample_stats[ph]["cells"] == m)
        np.testing.assert_array_equal(ps.sample_hist[ph], w["sample_hist"], err_msg=f"{store} phase {ph}: sample hist")
    # phase 1 started from the 4,096 cells of phase 0's sample
    for i in range(n):
        assert sum(want[0]["founders"][i].values()) == m


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 32), ("bins", 64)])
def test_phase_0_is_the_plain_run(engine_mod, store, kmax):
    for m in (40, 200, 4096):
        base = _base(store, kmax, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES)
        ps = engine_mod.run(_passage_spec(base, m)).passages
        plain = engine_mod.run(abi.RunSpec(**base, subsample_cells=m, stats_target=_targets()[0]))
        assert plain.passages is None
        for a, b in ((ps.summaries[0], plain.summaries), (ps.hist[0], plain.hist), (ps.totals[0], plain.totals),
                     (ps.stats[0], plain.stats), (ps.sample_stats[0], plain.sample_stats),
                     (ps.sample_hist[0], plain.sample_hist)):
            assert a.tobytes() == b.tobytes(), m


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax,m", [("rows", 0, 200), ("bins", 32, 40), ("bins", 64, 200)])
def test_chunks_and_shards(engine_mod, store, kmax, m, monkeypatch):
    base = _base(store, kmax, abi.BIRTH_DEATH, abi.SEG_BINOMIAL, BD_RATES)
    whole = engine_mod.run(_passage_spec(base, m)).passages
    names = ("summaries", "totals", "stats", "sample_stats", "hist", "sample_hist")
    hist = np.zeros_like(whole.hist)
    shist = np.zeros_like(whole.sample_hist)
    for gi in range(2):  # two interleaved shards
        part = engine_mod.run(_passage_spec(base, m, first_replicate=gi, replicate_stride=2, n_replicates=N // 2)).passages
        for f in ("summaries", "stats", "sample_stats"):
            assert getattr(part, f).tobytes() == np.ascontiguousarray(getattr(whole, f)[:, gi::2]).tobytes(), (gi, f)
        hist += part.hist
        shist += part.sample_hist
    np.testing.assert_array_equal(hist, whole.hist)
    np.testing.assert_array_equal(shist, whole.sample_hist)
    monkeypatch.setenv("ECDNA_SSA_MAX_CHUNK", "64")
    with engine_mod.Context(_passage_spec(base, m)) as ctx:
        assert ctx.instance()["n_chunks"] == 3 and ctx.row_stride() == 0
        ctx.launch()
        ssa_ms, hist_ms = ctx.sync()
        assert ssa_ms > 0.0 and hist_ms > 0.0  # summed over the (chunk, phase) pairs
        res = ctx.download()
    for f in names:
        assert getattr(res.passages, f).tobytes() == getattr(whole, f).tobytes(), f
    assert res.summaries.tobytes() == whole.summaries[G - 1].tobytes()


@pytest.mark.gpu
def test_download_passages_needs_a_passage_context(engine_mod):
    base = _base("rows", 0, abi.PURE_BIRTH, abi.SEG_BINOMIAL, PB_RATES)
    with engine_mod.Context(abi.RunSpec(**base)) as ctx:
        ctx.launch()
        ctx.sync()
        assert engine_mod.lib().ecdna_ssa_ctx_download_passages(ctx.h, None, None, None, None, None, None) == abi.E_STATE
    with engine_mod.Context(_passage_spec(base, 40)) as ctx:
        assert engine_mod.lib().ecdna_ssa_ctx_download_passages(ctx.h, None, None, None, None, None, None) == abi.E_STATE
        ctx.launch()
        assert engine_mod.lib().ecdna_ssa_ctx_download_passages(ctx.h, None, None, None, None, None, None) == abi.OK


# ------------------------------------------------------------------------------------------------------ joint law
# Pure birth, Binomial, from {1: 1} to max_cells = 4, m = 2, G = 2. A phase's final state is read from the per-phase
# outputs as (n-, n+, total copies = mean * cells); the joint table (phase 0, phase 1) is compared with the composition
# of tests/exact_law.py's enumeration of phase 0, the uniform 2-of-4 sample (each of the six pairs with probability
# 1/6: the hypergeometric law of the sample), and the enumeration from each founder state (Scenario expresses a
# founder state as an initial histogram).
JOINT_N = 1 << 18
JOINT_RATES = (1.0, 1.0, 0.0, 0.0)


def _scenario(init):
    return Scenario("passage-joint", abi.PURE_BIRTH, abi.SEG_BINOMIAL, JOINT_RATES, tuple(sorted(init.items())),
                    max_cells=4, max_iter=64, seed=5)


def _lump(law):
    """{(n-, n+, total copies): p} of a Law's final states."""
    out = {}
    for key, p in zip(law.keys, law.p):
        s = (int(key[1]), int(key[2]), int(key[6:].sum()))
        out[s] = out.get(s, 0.0) + float(p)
    return out


def _joint_law():
    from itertools import combinations

    law0 = enumerate_law(_scenario({1: 1}))
    joint = {}
    for key, p in zip(law0.keys, law0.p):
        nm, ks = int(key[1]), [int(k) for k in key[6:] if k > 0]
        s0 = (nm, len(ks), sum(ks))
        cells = [0] * nm + ks
        assert len(cells) == 4
        for pair in combinations(range(4), 2):
            init = {}
            for c in pair:
                init[cells[c]] = init.get(cells[c], 0) + 1
            for s1, p1 in _lump(enumerate_law(_scenario(init))).items():
                joint[(s0, s1)] = joint.get((s0, s1), 0.0) + float(p) * p1 / 6.0
    assert abs(sum(joint.values()) - 1.0) < 1e-9
    return joint


def _joint_pvalue(states0, states1):
    """chi2_lumped of the observed (phase-0 state, phase-1 state) pairs, [n][3] each, against the joint law."""
    law = _joint_law()
    keys = sorted(law)
    index = {k: i for i, k in enumerate(keys)}
    obs = np.zeros(len(keys) + 1)
    packed = np.concatenate([states0, states1], axis=1)
    rows, counts = np.unique(packed, axis=0, return_counts=True)
    for r, c in zip(rows.tolist(), counts.tolist()):
        obs[index.get((tuple(r[:3]), tuple(r[3:])), len(keys))] += c  # (the last cell: states the law cannot reach)
    exp = np.asarray([law[k] for k in keys] + [0.0]) * len(states0)
    return chi2_lumped(obs, exp, MIN_EXPECTED), obs, exp


def _states(summaries, ksum):
    return np.stack([summaries["nminus"].astype(np.int64), summaries["nplus"].astype(np.int64), ksum], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("store,kmax", [("rows", 0), ("bins", 32)])
def test_joint_law_of_two_phases(engine_mod, store, kmax):
    extra = dict(flags=abi.FLAG_BIN_STORE, bin_kmax=kmax) if store == "bins" else {}
    flags = abi.FLAG_REP_STATS | extra.pop("flags", 0)
    spec = _scenario({1: 1}).spec(n=JOINT_N, flags=flags, n_passages=2, passage_cells=2, **extra)
    ps = engine_mod.run(spec).passages
    assert np.all(ps.stats["cells"] == 4) and np.all(ps.sample_stats["cells"] == 2)
    ksum = np.rint(ps.stats["mean"] * 4).astype(np.int64)
    np.testing.assert_allclose(ps.stats["mean"] * 4, ksum, rtol=0, atol=1e-9)
    p, obs, exp = _joint_pvalue(_states(ps.summaries[0], ksum[0]), _states(ps.summaries[1], ksum[1]))
    assert obs[-1] == 0 and p > 1e-6, (p, obs.tolist(), exp.tolist())


def _founders_of_four(nminus, rows, seed, rids):
    """passage_law.founders for N = 4, m = 2, vectorised over the replicates: a Lemire draw below 4 never rejects
    ((2^32 - 4) mod 4 = 0) and is the first word's top two bits; the picks are u_0 and the first later u_i != u_0."""
    n = len(rids)
    cells = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        cells[i, int(nminus[i]):] = rows[i]

    def draw(i):
        return (sl.philox_blocks(i, sl.TAG, rids & np.uint64(0xFFFFFFFF), rids >> np.uint64(32), seed)[:, 0] >> np.uint64(30)).astype(np.int64)

    first = draw(0)
    second = np.full(n, -1, dtype=np.int64)
    i = 1
    while (second < 0).any():
        u = draw(i)
        take = (second < 0) & (u != first)
        second[take] = u[take]
        i += 1
        assert i < 4096
    a, b = cells[np.arange(n), first], cells[np.arange(n), second]
    return np.minimum(a, b), np.maximum(a, b)


def _oracle_joint(oracle_mod, phase1_seed):
    """The oracle's joint table, phase 1 run under `phase1_seed` (seed_1 is right; seed_0 replays phase 0's words)."""
    sc = _scenario({1: 1})
    n = JOINT_N
    o0 = oracle_mod.run(sc.spec(n=n), want_rows=True)
    rids = np.arange(n, dtype=np.uint64)
    rows = [o0.row(i) for i in range(n)]
    lo, hi = _founders_of_four(o0.summaries["nminus"], rows, sc.seed, rids)
    for i in range(0, n, n // 64):  # the vectorised founders are the restatement's
        nm, ks = pl.founders(int(o0.summaries[i]["nminus"]), rows[i], 2, sc.seed, 0, i)
        assert sorted([0] * nm + ks.tolist()) == [int(lo[i]), int(hi[i])], i
    inits = []
    for a, b in zip(lo.tolist(), hi.tolist()):
        h = {a: 1}
        h[b] = h.get(b, 0) + 1
        inits.append(h)
    spec1 = abi.RunSpec(process=sc.process, segregation=sc.segregation, rates=(JOINT_RATES,) * n, reps_per_set=1,
                        init_per_set=inits, max_cells=4, max_iter=64, max_time=float("inf"), seed=phase1_seed,
                        n_replicates=n, cell_cap=16, hist_bins=4, flags=0)
    o1 = oracle_mod.run(spec1, want_rows=True)
    k0 = np.asarray([int(r.sum()) for r in rows], dtype=np.int64)
    k1 = np.asarray([int(o1.row(i).sum()) for i in range(n)], dtype=np.int64)
    return _joint_pvalue(_states(o0.summaries, k0), _states(o1.summaries, k1))


def test_joint_law_has_power_against_a_replayed_key(oracle_mod):
    """On the CPU: the oracle chain under seed_1 fits the joint law, and the same chain with phase 1 wrongly run under
    seed_0 (the phase-0 words again: the founders' first events repeat their ancestors') is rejected below 1e-9 at
    2^18 replicates, so the GPU test above would see a stepper that ignored seed_g."""
    sc = _scenario({1: 1})
    p_right, obs, _ = _oracle_joint(oracle_mod, pl.seed_g(sc.seed, 1))
    assert obs[-1] == 0 and p_right > 1e-6, p_right
    p_wrong, _, _ = _oracle_joint(oracle_mod, sc.seed)
    assert p_wrong < 1e-9, p_wrong
