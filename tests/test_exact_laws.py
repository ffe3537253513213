"""The CPU oracle against exact laws (tests/exact_law.py), and the proof that the checker has power.

Every run here is the run tests/test_gpu_exact_laws.py makes on the GPU: same builder, same seed, same 2^20
replicates. The GPU's philox and reference-draws outputs are bit-identical to the oracle's (test_gpu_parity,
test_gpu_refdraws), so this file decides, without a GPU, whether each seeded GPU assertion passes. The oracle runs in
philox mode with the row store and the bin store at K = 32, 64 and 256, and in compat mode ("ref": ChaCha8, first
reaction, BINV/BTPE). Every p-value must exceed exact_law.P_MIN = 1e-6.

Measured here (2^20 replicates per run; "lowest p" is the lowest of a scenario's p-values over its tests and draw
paths; the MI355X column is the same minimum over all variants of tests/test_gpu_exact_laws.py, equal because the
engine's outputs equal the oracle's bit for bit). Enumeration times are of one CPU core.

  scenario           states  enum. s  lowest p  (test, path)
  bd_binomial         29593    0.28   0.157     mean_time, bins32
  pb_binomial         12628    0.07   0.0142    omnibus, bins32
  pb_no_nminus        67285    0.33   0.0156    mean_time, ref
  bd_no_uneven          968    0.01   0.0473    cells_k2, ref
  bd_deterministic      271    0.003  0.00598   cells_k1, bins32
  bd_extinction       59647    0.45   0.0507    mean_death_nplus, ref
  bd_cap_compat        5626    0.04   0.14      stop_x_cells, ref
  multi_set (4 sets: 29593 / 34850 / 855 / 570 states, 0.20 / 0.24 / 0.006 / 0.003 s)
                                      0.0229    set0/stop_x_cells, ref
  one-event and time-stop laws (closed forms, nothing enumerated):
  channel + time (3 populations x f64/f32)      0.0157    channel, population 1, ref
  split (14 copy numbers)                       0.0146    split_hist, k = 64, ref
  split, no-uneven (k = 1, 2, 3)                0.103     mean_k1, k = 3, rows
  pick (2^22 replicates)                        0.144     ref
  Yule time stop                                0.865     cells, rows
Some 2,000 p-values in all; the lowest is 0.006, as it should be for that many uniform draws. No seed was changed.

Power: the same row-store oracle data against deliberately wrong expected laws; the lowest marginal p-value (the
omnibus chi-square is left out) per data set. A wrong law counts as rejected below P_MIN / 1000 = 1e-9.
("0": below 1e-300, or a final state the wrong law cannot reach.)

  wrong law                  bd_binomial  bd_cap_compat  pb_no_nminus  one-event data
  b1 x 1.01                  3.3e-36      7.4e-35        1.9e-35       -
  pick 1 % toward larger k   0.095        0.14           0.037         pick, 2^22: 6.4e-18 (at 2^20: 2.2e-6)
  split p = 0.502            0.16         0.26           0.049         split k = 1: 0.028; 8: 2.7e-61; 32: 4.5e-230;
                                                                       257, 5000: 0
  uneven adds no N-          0            0              0.049 (*)     -
  cell stop one late         0            0              0             -
Every wrong law is rejected by at least one test. Two of them only by one-event data, and that is structural:
  * a final state keeps a division's daughters as a pair, whose law depends on (p - 1/2)^2: a split probability of
    0.502 moves the joint-state marginals by 4e-6 and only the row store's draw-ordered rows (k1 first) see it, from
    k = 8 up (at k = 1 every even split is (1, 1));
  * with copy numbers of 1 and 2 a pick biased by 1 % moves the joint-state marginals too little for 2^20
    replicates; the one-event pick among 1-, 2- and 70-copy cells sees it, and was raised to 2^22 replicates for
    that (at 2^20 it reached 2.2e-6 only).
  (*) the no-N- scenario's own rule adds no N- cell, so this wrong law is its true law.
"""
import pytest

import exact_law as X
from ecdna_evo_amd import abi

STORES = list(X.STORES)
_RUNS: dict = {}


def run_oracle(oracle_mod, spec, store, want_rows=True):
    return oracle_mod.run(spec, mode="compat" if store == "ref" else "philox", want_rows=want_rows)


def scenario_run(oracle_mod, name, store):
    """Joint-state runs are kept for the power tests (row store only) and otherwise dropped."""
    key = (name, store)
    if key in _RUNS:
        return _RUNS[key]
    sc = X.SCENARIOS[name]
    r = run_oracle(oracle_mod, X.scenario_spec(sc, store), store)
    if store == "rows":
        _RUNS[key] = r
    return r


# ------------------------------------------------------------------------------------------------ the enumerator

def test_enumerator_hand_computed_case():
    """Pure birth from one k = 1 cell to two cells, b1 = 0.5: one event after an Exp(1/2) wait; the cell splits
    (1, 1) or, with probability 2 * 2^-2 = 1/2, unevenly into one 2-copy cell and an N- cell."""
    sc = X.Scenario("hand", abi.PURE_BIRTH, abi.SEG_BINOMIAL, (1.0, 0.5, 0.0, 0.0), ((1, 1),), 2, 9)
    law = X.enumerate_law(sc)
    got = {tuple(k): p for k, p in zip(law.keys.tolist(), law.p)}
    assert got == {(abi.STOP_MAX_CELLS, 0, 2, 1, 0, 0, 1, 1): 0.5, (abi.STOP_MAX_CELLS, 1, 1, 1, 1, 0, 2, 0): 0.5}
    assert law.time_mean_var() == (2.0, 4.0)
    assert law.event_counts().tolist() == [[0, 1, 0, 0], [0, 1, 0, 0]]


def test_enumerator_birth_death_case_by_hand():
    """Birth-death from {1 N-, one k = 1 cell}, rates (1, 1, 0.5, 0.5), one event, no cell limit in reach:
    a0 = 3 and the first event is N- birth 1/3, N+ birth 1/3 (half of them uneven), N- death 1/6, N+ death 1/6."""
    sc = X.Scenario("hand2", abi.BIRTH_DEATH, abi.SEG_BINOMIAL, (1.0, 1.0, 0.5, 0.5), ((0, 1), (1, 1)), 9, 1)
    law = X.enumerate_law(sc)
    got = {tuple(k[:6]) + tuple(k[6:]): p for k, p in zip(law.keys.tolist(), law.p)}
    I = abi.STOP_MAX_ITER
    want = {(I, 2, 1, 1, 0, 0, 1, 0): 1 / 3, (I, 1, 2, 1, 0, 0, 1, 1): 1 / 6, (I, 2, 1, 1, 1, 0, 2, 0): 1 / 6,
            (I, 0, 1, 1, 0, 0, 1, 0): 1 / 6, (I, 1, 0, 1, 0, 1, 0, 0): 1 / 6}
    assert got.keys() == want.keys()
    assert all(abs(got[k] - want[k]) < 1e-15 for k in want)
    m, v = law.time_mean_var()
    assert abs(m - 1 / 3) < 1e-15 and abs(v - 1 / 9) < 1e-15
    by_key = dict(zip(map(tuple, law.keys.tolist()), law.event_counts().tolist()))
    assert by_key[(I, 2, 1, 1, 1, 0, 2, 0)] == [0, 1, 0, 0] and by_key[(I, 1, 0, 1, 0, 1, 0, 0)] == [0, 0, 0, 1]
    assert by_key[(I, 0, 1, 1, 0, 0, 1, 0)] == [0, 0, 1, 0] and by_key[(I, 2, 1, 1, 0, 0, 1, 0)] == [1, 0, 0, 0]


def test_scenarios_enumerate_within_the_budget_and_cover_the_model():
    laws = {n: X.enumerate_law(sc) for n, sc in X.SCENARIOS.items()}
    laws.update({sc.name: X.enumerate_law(sc) for sc in X.MULTI_SET})
    stops = set()
    for name, law in laws.items():
        print(f"ENUM {name} | {law.n_states} states | {law.transitions} transitions | {law.seconds:.3f} s")
        assert law.transitions <= X.MAX_TRANSITIONS
        assert law.width <= 7 and law.keys[:, X.EV].max() <= 8 and max(law.sc.cells0) <= 2
        stops |= set(law.keys[:, X.STOP].tolist())
    assert stops == {abi.STOP_MAX_CELLS, abi.STOP_MAX_ITER, abi.STOP_ABSORBING}
    scs = list(X.SCENARIOS.values())
    assert {s.process for s in scs} == {abi.PURE_BIRTH, abi.BIRTH_DEATH}
    assert {s.segregation for s in scs} == set(abi.SEGREGATION_NAMES.values())
    assert any(s.cap_compat for s in scs)
    assert any(s.rates[0] > s.rates[1] for s in scs) and any(s.rates[0] < s.rates[1] for s in scs)
    ext = laws["bd_extinction"]
    assert ext.p[ext.keys[:, X.STOP] == abi.STOP_ABSORBING].sum() > 0.5


def test_enumerator_rejects_a_scenario_beyond_its_budget(monkeypatch):
    """Four 2-copy cells and 8 events are millions of states: rejected at the transition budget (checked here at a
    hundredth of it, so that the rejection itself stays quick)."""
    monkeypatch.setattr(X, "MAX_TRANSITIONS", X.MAX_TRANSITIONS // 100)
    with pytest.raises(X.ScenarioTooLarge):
        X.enumerate_law(X.Scenario("too_large", abi.BIRTH_DEATH, abi.SEG_BINOMIAL_NO_NMINUS, X.NPLUS_FITTER,
                                   ((2, 4),), 12, 8))


# ------------------------------------------------------------------------------- the oracle against the exact laws

@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("name", sorted(X.SCENARIOS))
def test_oracle_joint_state_law(name, store, oracle_mod):
    law = X.enumerate_law(X.SCENARIOS[name])
    X.assert_laws(X.check_sets([law], scenario_run(oracle_mod, name, store)), f"{name}/{store}")


@pytest.mark.parametrize("store", STORES)
def test_oracle_multi_set_law(store, oracle_mod):
    laws = [X.enumerate_law(sc) for sc in X.MULTI_SET]
    X.assert_laws(X.check_sets(laws, run_oracle(oracle_mod, X.scenario_spec(X.MULTI_SET, store), store)),
                f"multi_set/{store}")


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("store", STORES)
def test_oracle_one_event_channel_and_time(store, f32, oracle_mod):
    for i in range(len(X.CHANNEL_POPS)):
        r = run_oracle(oracle_mod, X.channel_spec(i, store, f32), store, want_rows=False)
        X.assert_laws(X.check_channel(r, i), f"channel{i}/{store}/f32={int(f32)}")


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("k", X.SPLIT_KS)
def test_oracle_one_event_split(k, store, oracle_mod):
    ordered = store in ("rows", "ref")
    r = run_oracle(oracle_mod, X.split_spec(k, store), store, want_rows=X.split_needs_rows(k, store))
    if store == "rows":
        _RUNS[("split", k)] = r
    X.assert_laws(X.check_split(r, k, ordered_rows=ordered), f"split{k}/{store}")


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("k", X.NO_UNEVEN_KS)
def test_oracle_one_event_split_no_uneven(k, store, oracle_mod):
    ordered = store in ("rows", "ref")
    r = run_oracle(oracle_mod, X.split_spec(k, store, no_uneven=True), store, want_rows=ordered)
    X.assert_laws(X.check_split(r, k, no_uneven=True, ordered_rows=ordered), f"split_no_uneven{k}/{store}")


@pytest.mark.parametrize("store", ["rows", "bins32", "bins64", "ref"])
def test_oracle_one_event_pick(store, oracle_mod):
    counts = [X.picked_counts(run_oracle(oracle_mod, spec, store)) for spec in X.pick_specs(store)]
    if store == "rows":
        _RUNS[("pick",)] = counts
    X.assert_laws(X.check_pick(counts), f"pick/{store}")


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("store", STORES)
def test_oracle_yule_time_stop(store, f32, oracle_mod):
    """Confirms the closed form's off-by-one (final cells = N(t) + 1) on every draw path before the GPU relies on it."""
    r = run_oracle(oracle_mod, X.yule_spec(store, f32), store, want_rows=False)
    X.assert_laws(X.check_yule(r), f"yule/{store}/f32={int(f32)}")


# ------------------------------------------------------------------------------------------------ power self-tests

REJECT = X.P_MIN * 1e-3  # a wrong law must sit at least three decades below the acceptance threshold
# the scenarios whose wrong chains stay within the enumeration budget under every perturbation (a wrong rule that adds
# no cell, or stops later, lets the other chains grow past it)
POWER_SCENARIOS = ["bd_binomial", "bd_cap_compat", "pb_no_nminus"]


@pytest.mark.parametrize("what", X.PERTURBATIONS)
def test_wrong_law_is_rejected(what, oracle_mod):
    """The oracle's own row-store data (the GPU tests' seeds and sizes) against a deliberately wrong expected law:
    at least one marginal test (never the omnibus chi-square) must reject it below P_MIN / 1000. The lowest p-value
    per scenario is printed; the module docstring tabulates them."""
    lowest = {}
    for name in POWER_SCENARIOS:
        wrong = X.perturbed_law(X.SCENARIOS[name], what)
        ps = X.check_sets([wrong], scenario_run(oracle_mod, name, "rows"), want_rows=False)
        worst = min(ps, key=ps.get)
        lowest[name] = (ps[worst], worst)
    if what == "split p = 0.502":
        # final states keep the daughters as a pair, and the law of the pair depends on (p - 1/2)^2 only: the joint
        # scenarios cannot see this error. The row store's one-event split keeps the draw order.
        for k in (1, 8, 32, 257, 5000):
            r = _RUNS.get(("split", k)) or run_oracle(oracle_mod, X.split_spec(k, "rows"), "rows")
            ps = X.check_split(r, k, ordered_rows=True, split_p=0.502)
            worst = min(ps, key=ps.get)
            lowest[f"split k={k}"] = (ps[worst], worst)
    if what == "pick 1 % toward larger k":
        counts = _RUNS.get(("pick",)) or [X.picked_counts(run_oracle(oracle_mod, spec, "rows"))
                                          for spec in X.pick_specs("rows")]
        lowest["one-event pick"] = (X.check_pick(counts, pick_bias=0.01)["pick"], "pick")
    for name, (p, test) in lowest.items():
        print(f"POWER {what} | {name} | {test} | {p:.3g}")
    assert min(p for p, _ in lowest.values()) < REJECT, lowest


def test_true_law_is_accepted_where_the_wrong_ones_are_rejected(oracle_mod):
    """The same data and the same marginals against the true law: all accepted (the rejections above are the wrong
    laws' doing, not the checker's)."""
    for name in POWER_SCENARIOS:
        ps = X.check_sets([X.enumerate_law(X.SCENARIOS[name])], scenario_run(oracle_mod, name, "rows"), want_rows=False)
        assert min(ps.values()) > X.P_MIN, (name, ps)
