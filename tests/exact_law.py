"""Exact small-population laws of the ecDNA birth(-death) process: the reference the law tests compare with.

Nothing here shares code with `oracle/` or `csrc/`: the enumerator is written from the model's definition
(SURVEY.md App. A.3 and DESIGN.md §3.1, which cite src/process.rs and src/proliferation.rs:25-139) in plain Python,
in float64, and imports only constants (and the RunSpec builder) from `ecdna_evo_amd.abi`.

The process, per iteration, in this order:
  1. stop with MaxIter when `events >= max_iter`;
  2. stop with MaxCells when `(n- + n+) * m >= max_cells` (m = 2 for birth-death under FLAG_BD_CAP_COMPAT, else 1);
  3. stop with Absorbing when the total propensity is 0;
  4. draw the channel with probability proportional to [b0 n-, b1 n+, d0 n-, d1 n+] (pure birth: the first two)
     and add an independent Exp(a0) to the clock.
An N+ birth picks a uniform N+ cell of k copies and splits n = 2k copies with k1 ~ Bin(n, 1/2): daughters
(k1, n - k1); when k1 is 0 or n ("uneven") one cell of n copies plus one N- cell; NO_NMINUS: the same without the
N- cell (still counted as uneven); NO_UNEVEN: k1 conditioned on 0 < k1 < n; DETERMINISTIC: (k, k). An N+ death
removes a uniform N+ cell. (The time stop is not enumerated: `max_time` is infinite in every enumerated scenario;
the Yule closed form below covers it.)

With a handful of cells and a small event cap this is a finite Markov chain. `enumerate_law` walks it forward,
layer by layer (one layer per event), and carries (p, E[T 1], E[T^2 1]) per state, so the exact mean and variance
of the final time come out with the law of the final state. The state is (n-, sorted N+ copy numbers, uneven
count, N+ deaths); the event count is the layer. The N+ death count rides along so that the four per-channel event
counts are functions of the final state (`Law.event_counts`):
    c3 = deaths of N+;  c1 = n+ - n+(0) + uneven + c3;  c0 + c2 = events - c1 - c3;
    c0 - c2 = n- - n-(0) - (uneven under BINOMIAL, else 0).

Rates must be exactly representable in f32 (1, 1.5, 0.25, 0.5, ...), so the engine's f32 propensities
rate * population are exact for these populations and add no model error.

A scenario is rejected (`ScenarioTooLarge`) when its enumeration needs more than `MAX_TRANSITIONS` transitions:
that is the deterministic form of "finishes in under a second" (the largest scenario here takes 0.45 s of one CPU
core; the measured times are in the docstring of tests/test_exact_laws.py). Copy numbers double at every
division, so joint-state scenarios stay at k <= 2, about 7 cells and 6-8 events; large k is tested by one-event
laws (closed forms below).

Test statistics (all return a p-value):
  * `chi2_lumped`: Pearson chi-square with the cells of expected count < 20 lumped into one; an observation where
    the law has probability 0 gives p = 0;
  * `z_pvalue`: two-sided z-test of a mean against the exact mean and per-replicate variance;
  * `binom_pvalue`: exact binomial test of one proportion;
  * `ks_exp_pvalue`: Kolmogorov-Smirnov against Exp(a0). The engine's clock is a 23-bit soft log, so its one-event
    times sit on a grid of 2^23 points and the KS statistic carries a discretisation of up to 2^-23 = 1.2e-7, far
    below its resolution 1 / sqrt(N) = 1e-3 at N = 2^20; the exact-distribution p-value is used unchanged.
Observed states are counted vectorised (`np.unique` over a packed matrix); there is no Python loop over replicates.
"""
from __future__ import annotations

import math
import time
from collections import Counter
from dataclasses import dataclass, replace
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
from scipy import stats

from ecdna_evo_amd import abi

P_MIN = 1e-6  # acceptance threshold of every law assertion (|z| < 4.9)
N_REPLICATES = 1 << 20
MIN_EXPECTED = 20.0
MAX_TRANSITIONS = 600_000

# columns of a packed state matrix (law keys and observed replicates alike); the sorted N+ row follows
STOP, NM, NP, EV, UN, D3 = range(6)
N_HEAD = 6


class ScenarioTooLarge(ValueError):
    pass


@dataclass(frozen=True)
class Scenario:
    name: str
    process: int
    segregation: int
    rates: Tuple[float, float, float, float]
    init: Tuple[Tuple[int, int], ...]  # ((copies, cells), ...); copies 0 = N- cells
    max_cells: int
    max_iter: int
    cap_compat: bool = False
    seed: int = 1

    def __post_init__(self):
        for r in self.rates:
            if float(np.float32(r)) != float(r):
                raise ValueError(f"rate {r} is not exactly representable in f32")

    @property
    def nminus0(self) -> int:
        return sum(c for k, c in self.init if k == 0)

    @property
    def cells0(self) -> Tuple[int, ...]:
        return tuple(sorted(k for k, c in self.init if k > 0 for _ in range(c)))

    @property
    def flags(self) -> int:
        return abi.FLAG_BD_CAP_COMPAT if self.cap_compat else 0

    def spec(self, n: int = N_REPLICATES, flags: int = 0, **kw) -> "abi.RunSpec":
        """The run of this scenario: max_time infinite (RunSpec's default is floor(log2(cells) + 4)), cell_cap 16,
        a 4-bin histogram (k = 0, 1, 2, >= 3)."""
        kw.setdefault("cell_cap", 16)
        kw.setdefault("hist_bins", 4)
        return abi.RunSpec(process=self.process, segregation=self.segregation, rates=(self.rates,),
                           init=dict(self.init), max_cells=self.max_cells, max_iter=self.max_iter,
                           max_time=float("inf"), seed=self.seed, n_replicates=n, flags=self.flags | flags, **kw)


def multi_set_spec(scs: Sequence[Scenario], n: int = N_REPLICATES, flags: int = 0, **kw) -> "abi.RunSpec":
    """One launch of len(scs) parameter sets (rates and initial distribution per set); n replicates in all."""
    a = scs[0]
    assert all((s.process, s.segregation, s.max_cells, s.max_iter, s.cap_compat) ==
               (a.process, a.segregation, a.max_cells, a.max_iter, a.cap_compat) for s in scs)
    assert n % len(scs) == 0
    kw.setdefault("cell_cap", 16)
    kw.setdefault("hist_bins", 4)
    return abi.RunSpec(process=a.process, segregation=a.segregation, rates=tuple(s.rates for s in scs),
                       init_per_set=[dict(s.init) for s in scs], reps_per_set=n // len(scs), max_cells=a.max_cells,
                       max_iter=a.max_iter, max_time=float("inf"), seed=a.seed, n_replicates=n,
                       flags=a.flags | flags, **kw)


# ------------------------------------------------------------------------------------------------ the enumerator

def _split_law(k: int, seg: int, p: float, uneven_adds_nminus: bool):
    """The daughters of a k-copy cell: [(probability, daughters, N- cells added, uneven events added)]."""
    n = 2 * k
    if seg == abi.SEG_DETERMINISTIC:
        return [(1.0, (k, k), 0, 0)]
    if p == 0.5:
        pmf = [math.comb(n, j) / 2.0 ** n for j in range(n + 1)]
    else:
        pmf = stats.binom.pmf(np.arange(n + 1), n, p).tolist()
    even: Dict[Tuple[int, int], float] = {}
    for j in range(1, n):
        d = (min(j, n - j), max(j, n - j))
        even[d] = even.get(d, 0.0) + pmf[j]
    pu = pmf[0] + pmf[n]
    if seg == abi.SEG_BINOMIAL_NO_UNEVEN:
        return [(q / (1.0 - pu), d, 0, 0) for d, q in even.items()]
    out = [(q, d, 0, 0) for d, q in even.items()]
    adds = 1 if (seg == abi.SEG_BINOMIAL and uneven_adds_nminus) else 0
    out.append((pu, (n,), adds, 1))
    return out


class _Chain:
    def __init__(self, sc: Scenario, split_p: float, pick_bias: float, uneven_adds_nminus: bool):
        self.sc, self.split_p, self.pick_bias, self.adds = sc, split_p, pick_bias, uneven_adds_nminus
        self.bd = sc.process == abi.BIRTH_DEATH
        self.cache: dict = {}
        self.splits: dict = {}
        self.work = 0

    def pick(self, ks):
        """[(probability, k, the other cells)]: uniform over cells; `pick_bias` (a deliberately wrong law for the
        power tests) weights the cells of the largest copy number by 1 + pick_bias when the copy numbers differ."""
        cnt = Counter(ks)
        top = max(cnt)
        w = {k: c * ((1.0 + self.pick_bias) if (k == top and len(cnt) > 1) else 1.0) for k, c in cnt.items()}
        tot = sum(w.values())
        out = []
        for k in cnt:
            rest = list(ks)
            rest.remove(k)
            out.append((w[k] / tot, k, rest))
        return out

    def transitions(self, nm: int, ks: tuple):
        key = (nm, ks)
        hit = self.cache.get(key)
        if hit is not None:
            return hit
        b0, b1, d0, d1 = self.sc.rates
        n_plus = len(ks)
        a = [b0 * nm, b1 * n_plus] + ([d0 * nm, d1 * n_plus] if self.bd else [])
        a0 = sum(a)
        acc: Dict[tuple, float] = {}
        if a0 > 0.0:
            if a[0] > 0.0:
                acc[(nm + 1, ks, 0, 0)] = a[0] / a0
            if a[1] > 0.0:
                for pk, k, rest in self.pick(ks):
                    sl = self.splits.get(k)
                    if sl is None:
                        sl = self.splits[k] = _split_law(k, self.sc.segregation, self.split_p, self.adds)
                    for ps, d, dnm, du in sl:
                        t = (nm + dnm, tuple(sorted(rest + list(d))), du, 0)
                        acc[t] = acc.get(t, 0.0) + a[1] / a0 * pk * ps
            if self.bd and a[2] > 0.0:
                acc[(nm - 1, ks, 0, 0)] = a[2] / a0
            if self.bd and a[3] > 0.0:
                for pk, k, rest in self.pick(ks):
                    t = (nm, tuple(rest), 0, 1)
                    acc[t] = acc.get(t, 0.0) + a[3] / a0 * pk
        res = (a0, [(q,) + t for t, q in acc.items()])
        self.cache[key] = res
        return res


class Law:
    """The exact law of a scenario's final state: `keys` [S][6 + W] (stop, n-, n+, events, uneven, N+ deaths, the N+
    copy numbers sorted descending and zero-padded), with p, E[T 1] and E[T^2 1] per final state."""

    def __init__(self, sc: Scenario, final: dict, seconds: float, transitions: int):
        self.sc, self.seconds, self.transitions = sc, seconds, transitions
        W = max(len(k[5]) for k in final)
        keys = np.zeros((len(final), N_HEAD + W), dtype=np.int64)
        vals = np.zeros((len(final), 3))
        for i, ((stop, nm, ev, u, d3, ks), v) in enumerate(final.items()):
            keys[i, :N_HEAD] = (stop, nm, len(ks), ev, u, d3)
            keys[i, N_HEAD:N_HEAD + len(ks)] = ks[::-1]
            vals[i] = v
        self.keys, self.p, self.t1, self.t2 = keys, vals[:, 0], vals[:, 1], vals[:, 2]
        self.width = W
        self.n_states = len(final)
        assert abs(self.p.sum() - 1.0) < 1e-12, self.p.sum()

    def time_mean_var(self):
        m = float(self.t1.sum())
        return m, float(self.t2.sum()) - m * m

    def event_counts(self, keys: Optional[np.ndarray] = None) -> np.ndarray:
        """[S][4] events by channel, from the identities in the module docstring."""
        K = self.keys if keys is None else keys
        sc = self.sc
        c3 = K[:, D3]
        c1 = K[:, NP] - len(sc.cells0) + K[:, UN] + c3
        rest = K[:, EV] - c1 - c3
        diff = K[:, NM] - sc.nminus0 - (K[:, UN] if sc.segregation == abi.SEG_BINOMIAL else 0)
        return np.stack([(rest + diff) // 2, c1, (rest - diff) // 2, c3], axis=1)

    def cells_by_k(self) -> np.ndarray:
        """[S][4] cells with 0 (N-), 1, 2 and >= 3 copies."""
        R = self.keys[:, N_HEAD:]
        return np.stack([self.keys[:, NM], (R == 1).sum(1), (R == 2).sum(1), (R >= 3).sum(1)], axis=1)

    def moments(self, x: np.ndarray):
        """Mean and variance of a function of the final state (x: [S])."""
        m = float((self.p * x).sum())
        return m, max(0.0, float((self.p * x * x).sum()) - m * m)

    def chi2(self, observed, cols: Optional[Sequence[int]] = None) -> float:
        """Lumped chi-square of the observed replicates (`count_rows` of their packed matrix: distinct rows and how
        often each occurs) against this law, over the given columns (None: every column, the omnibus final-state
        test)."""
        A, (B, counts) = self.keys, observed
        if cols is None:
            w = max(A.shape[1], B.shape[1])
            A = np.pad(A, ((0, 0), (0, w - A.shape[1])))
            B = np.pad(B, ((0, 0), (0, w - B.shape[1])))
        else:
            A, B = A[:, list(cols)], B[:, list(cols)]
        ids = _labels(A, B)
        S = len(A)
        m = int(ids.max()) + 1
        prob = np.bincount(ids[:S], weights=self.p, minlength=m)
        obs = np.bincount(ids[S:], weights=counts, minlength=m)
        return chi2_lumped(obs, prob * counts.sum())


def _words(M: np.ndarray):
    """The rows of an integer matrix packed, mixed radix, into as few int64 words per row as they need."""
    lo = M.min(0)
    span = M.max(0) - lo + 1
    words, cur, cap = [], None, 1
    for c in range(M.shape[1]):
        s = int(span[c])
        if cur is not None and cap * s >= (1 << 62):
            words.append(cur)
            cur, cap = None, 1
        col = M[:, c] - lo[c]
        cur = col.copy() if cur is None else cur * s + col
        cap *= s
    words.append(cur)
    return words


def _row_ids(M: np.ndarray) -> np.ndarray:
    """Labels of the rows of M: equal rows get equal labels (the packed words merged through `np.unique`)."""
    words = _words(M.astype(np.int64))
    ids = np.unique(words[0], return_inverse=True)[1].astype(np.int64).ravel()
    for wd in words[1:]:
        u, inv = np.unique(wd, return_inverse=True)
        ids = np.unique(ids * len(u) + inv.ravel(), return_inverse=True)[1].astype(np.int64).ravel()
    return ids


def count_rows(M: np.ndarray):
    """(distinct rows of M, their counts): the one pass over all replicates; the tests then work on distinct rows."""
    ids = _row_ids(M)
    _, first, counts = np.unique(ids, return_index=True, return_counts=True)
    return M[first], counts.astype(np.float64)


def _labels(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """Row labels of the stacked integer matrices [A; B]."""
    return _row_ids(np.concatenate([A, B]))


_LAWS: dict = {}


def enumerate_law(sc: Scenario, split_p: float = 0.5, pick_bias: float = 0.0, uneven_adds_nminus: bool = True,
                  cells_stop_late: int = 0) -> Law:
    """The exact law of `sc` (cached per scenario). The keyword arguments make deliberately WRONG laws for the power
    self-tests: a split probability other than 1/2, a pick weighted toward the largest copy number, an uneven split
    that adds no N- cell, and a cell-count stop `cells_stop_late` cells late."""
    ck = (sc, split_p, pick_bias, uneven_adds_nminus, cells_stop_late)
    if ck in _LAWS:
        return _LAWS[ck]
    t0 = time.perf_counter()
    ch = _Chain(sc, split_p, pick_bias, uneven_adds_nminus)
    m = 2 if (sc.cap_compat and ch.bd) else 1
    live = {(sc.nminus0, sc.cells0, 0, 0): (1.0, 0.0, 0.0)}
    final: dict = {}
    ev = work = 0
    while live:
        nxt: dict = {}
        for (nm, ks, u, d3), (p, t1, t2) in live.items():
            stop = 0
            if ev >= sc.max_iter:
                stop = abi.STOP_MAX_ITER
            elif (nm + len(ks)) * m >= sc.max_cells + cells_stop_late * m:
                stop = abi.STOP_MAX_CELLS
            else:
                a0, trs = ch.transitions(nm, ks)
                if a0 == 0.0:
                    stop = abi.STOP_ABSORBING
            if stop:
                fk = (stop, nm, ev, u, d3, ks)
                q = final.get(fk)
                final[fk] = (p, t1, t2) if q is None else (q[0] + p, q[1] + t1, q[2] + t2)
                continue
            # an independent X ~ Exp(a0) is added: E[(T + X) 1] = E[T 1] + p / a0 and
            # E[(T + X)^2 1] = E[T^2 1] + 2 E[T 1] / a0 + 2 p / a0^2
            inv = 1.0 / a0
            n1, n2 = t1 + p * inv, t2 + 2.0 * t1 * inv + 2.0 * p * inv * inv
            work += len(trs)
            for q, nm2, ks2, du, dd in trs:
                nk = (nm2, ks2, u + du, d3 + dd)
                o = nxt.get(nk)
                nxt[nk] = (p * q, n1 * q, n2 * q) if o is None else (o[0] + p * q, o[1] + n1 * q, o[2] + n2 * q)
        if work > MAX_TRANSITIONS:
            raise ScenarioTooLarge(f"{sc.name}: more than {MAX_TRANSITIONS} transitions at event {ev}")
        live = nxt
        ev += 1
    law = Law(sc, final, time.perf_counter() - t0, work)
    _LAWS[ck] = law
    return law


# --------------------------------------------------------------------------------------------------- statistics

def chi2_lumped(obs: np.ndarray, exp: np.ndarray, min_expected: float = MIN_EXPECTED) -> float:
    obs = np.asarray(obs, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    if np.any((exp <= 0.0) & (obs > 0)):
        return 0.0  # a state the law cannot reach
    big = exp >= min_expected
    o, e = list(obs[big]), list(exp[big])
    lo, le = float(obs[~big].sum()), float(exp[~big].sum())
    if le > 0.0:
        if le >= 5.0 or not e:
            o.append(lo)
            e.append(le)
        else:  # too small for a cell of its own: joins the smallest remaining cell
            j = int(np.argmin(e))
            o[j] += lo
            e[j] += le
    o, e = np.asarray(o), np.asarray(e)
    if len(e) < 2:
        return 1.0
    e = e * (o.sum() / e.sum())
    return float(stats.chi2.sf(((o - e) ** 2 / e).sum(), len(e) - 1))


def z_pvalue(observed_mean: float, mean: float, var: float, n: int) -> float:
    if var <= 0.0:
        return 1.0 if abs(observed_mean - mean) <= 1e-12 * max(1.0, abs(mean)) else 0.0
    return float(2.0 * stats.norm.sf(abs(observed_mean - mean) / math.sqrt(var / n)))


def binom_pvalue(x: int, n: int, p: float) -> float:
    return float(stats.binomtest(int(x), int(n), p).pvalue)


def ks_exp_pvalue(times: np.ndarray, a0: float) -> float:
    return float(stats.kstest(np.asarray(times, dtype=np.float64), stats.expon(scale=1.0 / a0).cdf).pvalue)


# ------------------------------------------------------------------------------------------- observed replicates

def pack_observed(summ: np.ndarray, rows: Optional[np.ndarray], width: int) -> np.ndarray:
    """The packed state matrix of a run's replicates: (stop, n-, n+, events, uneven, N+ deaths) and, with rows, each
    replicate's N+ copy numbers sorted descending, zero-padded to at least `width` columns."""
    head = np.stack([summ["stop_reason"].astype(np.int64), summ["nminus"].astype(np.int64),
                     summ["nplus"].astype(np.int64), summ["iters"].astype(np.int64),
                     summ["uneven"].astype(np.int64), summ["events_by_type"][:, 3].astype(np.int64)], axis=1)
    if rows is None:
        return head
    n_plus = summ["nplus"].astype(np.int64)
    w = min(rows.shape[1], max(width, int(n_plus.max(initial=0))))
    r = rows[:, :w].astype(np.int64)
    r[np.arange(w)[None, :] >= n_plus[:, None]] = 0
    r = -np.sort(-r, axis=1)
    return np.concatenate([head, r], axis=1)


def check_law(law: Law, summ: np.ndarray, hist: np.ndarray, totals: np.ndarray,
              rows: Optional[np.ndarray] = None) -> Dict[str, float]:
    """Every marginal test of one scenario (one parameter set) as {name: p-value}: summaries `summ` [n], the set's
    pooled 4-bin histogram `hist`, the set's totals record `totals`, and optionally the final rows [n][>= W]."""
    n = len(summ)
    out: Dict[str, float] = {}
    ok = int(totals["replicates"]) == n and int(totals["errors"]) == 0 and not summ["error"].any()
    out["no_errors"] = 1.0 if ok else 0.0
    M = count_rows(pack_observed(summ, rows, law.width))
    out["stop_x_cells"] = law.chi2(M, (STOP, NM, NP))
    out["events"] = law.chi2(M, (EV,))
    C = law.event_counts()
    names = ("prolif_nminus", "prolif_nplus", "death_nminus", "death_nplus")
    for j in range(4):
        mean, var = law.moments(C[:, j].astype(np.float64))
        out[f"mean_{names[j]}"] = z_pvalue(float(totals["events_by_type"][j]) / n, mean, var, n)
    mean, var = law.moments(law.keys[:, UN].astype(np.float64))
    out["mean_uneven"] = z_pvalue(float(totals["uneven"]) / n, mean, var, n)
    # the device-side totals are the sums of the per-replicate summaries
    sums_ok = (np.array_equal(summ["events_by_type"].sum(0), totals["events_by_type"])
               and int(summ["uneven"].sum()) == int(totals["uneven"])
               and int(summ["iters"].sum()) == int(totals["events"]))
    out["totals_are_sums"] = 1.0 if sums_ok else 0.0
    H = law.cells_by_k()
    assert len(hist) == 4, "the law tests read a 4-bin histogram (k = 0, 1, 2, >= 3)"
    for j, nm in enumerate(("k0", "k1", "k2", "k3plus")):
        mean, var = law.moments(H[:, j].astype(np.float64))
        out[f"cells_{nm}"] = z_pvalue(float(hist[j]) / n, mean, var, n)
    mean, var = law.time_mean_var()
    out["mean_time"] = z_pvalue(float(summ["time"].mean()), mean, var, n)
    if rows is not None:
        out["omnibus"] = law.chi2(M, None)
    return out


def check_sets(laws: Sequence[Law], res, want_rows: bool = True) -> Dict[str, float]:
    """check_law per parameter set of a run whose replicates are laid out set after set (reps_per_set each)."""
    n = len(res.summaries) // len(laws)
    out: Dict[str, float] = {}
    for s, law in enumerate(laws):
        sl = slice(s * n, (s + 1) * n)
        rows = res.rows[sl] if (want_rows and res.rows is not None) else None
        for k, v in check_law(law, res.summaries[sl], res.hist[s], res.totals[s], rows).items():
            out[f"{law.sc.name}/{k}" if len(laws) > 1 else k] = v
    return out


# ------------------------------------------------------------------------------------------------- closed forms

def split_pvalue(k1: np.ndarray, k: int, no_uneven: bool = False, folded: bool = False, p: float = 0.5) -> float:
    """chi-square of the observed first daughters k1 of a k-copy cell against Binomial(2k, 1/2). The uneven
    outcomes 0 and 2k are one class (the final state does not tell them apart); `folded` tests min(k1, 2k - k1)
    (a sorted row keeps the pair, not its order); `no_uneven` conditions on 0 < k1 < 2k."""
    n = 2 * k
    j = np.arange(n + 1)
    pmf = stats.binom.pmf(j, n, p)  # (p other than 1/2: a deliberately wrong law for the power tests)
    cls = j.copy()
    cls[n] = 0
    if folded:
        cls = np.minimum(cls, n - cls)
        cls[0] = cls[n] = 0
    if no_uneven:
        pmf[0] = pmf[n] = 0.0
        pmf /= pmf.sum()
    x = np.asarray(k1, dtype=np.int64)
    if np.any((x < 0) | (x > n)):
        return 0.0
    exp = np.bincount(cls, weights=pmf, minlength=n + 1) * len(x)
    obs = np.bincount(cls[x], minlength=n + 1)
    return chi2_lumped(obs, exp)


def split_pvalue_from_hist(hist: np.ndarray, nminus_total: int, k: int, n_reps: int, no_uneven: bool = False) -> float:
    """The same law read off the pooled copy-number histogram after one division of one k-copy cell in each of
    n_reps replicates: bins j < k and 2k - j each hold the replicates with min(k1, 2k - k1) = j, bin k twice those with
    k1 = k, bin 2k (and the N- bin) the uneven ones."""
    n = 2 * k
    h = np.asarray(hist, dtype=np.int64)
    if len(h) <= n or h[n + 1:].any() or h[k] % 2 or int(h[0]) != int(nminus_total):
        return 0.0
    if not np.array_equal(h[1:k], h[n - 1:k:-1]):  # every daughter of j < k copies has a sister of 2k - j
        return 0.0
    counts = np.concatenate([h[1:k], [h[k] // 2]])  # min = 1 .. k
    if int(counts.sum()) + int(h[n]) != n_reps or int(h[0]) != int(h[n]):
        return 0.0
    folded = np.repeat(np.concatenate([[0], np.arange(1, k + 1)]), np.concatenate([[h[n]], counts]))
    return split_pvalue(folded, k, no_uneven=no_uneven, folded=True)


def yule_stop_pvalue(cells: np.ndarray, t: float) -> float:
    """Pure birth, b0 = b1 = 1, from one cell, stopped at the first stop test at or past time t: the population at
    time t is geometric, P(N(t) = n) = e^-t (1 - e^-t)^(n-1), and one more event has happened by the stop test that
    sees the clock past t, so P(final cells = n + 1) = e^-t (1 - e^-t)^(n-1), n >= 1."""
    x = np.asarray(cells, dtype=np.int64)
    if x.min() < 2:
        return 0.0
    top = int(max(x.max(), 64))
    n = np.arange(1, top)  # final cells n + 1 = 2 .. top
    pmf = math.exp(-t) * (1.0 - math.exp(-t)) ** (n - 1.0)
    exp = np.concatenate([[0.0, 0.0], pmf]) * len(x)
    return chi2_lumped(np.bincount(x, minlength=top + 1), exp)


# ---------------------------------------------------------------------------------------------------- scenarios

BD, PB = abi.BIRTH_DEATH, abi.PURE_BIRTH
NPLUS_FITTER = (1.0, 1.5, 0.25, 0.5)
NMINUS_FITTER = (1.5, 1.0, 0.5, 0.25)

SCENARIOS = {s.name: s for s in [
    # birth-death, binomial, N+ fitter: stops by max_iter, by max_cells and (both cells dying) absorbing
    Scenario("bd_binomial", BD, abi.SEG_BINOMIAL, NPLUS_FITTER, ((1, 1), (2, 1)), 6, 6, seed=101),
    # pure birth to 7 cells, N- fitter: every run stops by max_cells after exactly 6 events
    Scenario("pb_binomial", PB, abi.SEG_BINOMIAL, (1.5, 1.0, 0.0, 0.0), ((1, 1),), 7, 64, seed=102),
    # the no-N- rule: an uneven split doubles the cell and adds nothing; stops by max_iter and max_cells
    Scenario("pb_no_nminus", PB, abi.SEG_BINOMIAL_NO_NMINUS, (1.0, 1.5, 0.0, 0.0), ((0, 1), (1, 2)), 6, 7, seed=103),
    # the no-uneven rule with deaths, N- fitter (N- cells only from the start)
    Scenario("bd_no_uneven", BD, abi.SEG_BINOMIAL_NO_UNEVEN, NMINUS_FITTER, ((0, 1), (1, 2), (2, 1)), 7, 6, seed=104),
    Scenario("bd_deterministic", BD, abi.SEG_DETERMINISTIC, NPLUS_FITTER, ((0, 1), (1, 2), (2, 1)), 7, 8, seed=105),
    # extinction-prone: deaths outrun births, most runs end absorbing
    Scenario("bd_extinction", BD, abi.SEG_BINOMIAL, (0.5, 1.0, 1.5, 1.5), ((1, 1), (2, 1)), 6, 7, seed=106),
    # the halved birth-death cell limit: stops at 6 cells under max_cells = 12
    Scenario("bd_cap_compat", BD, abi.SEG_BINOMIAL, NPLUS_FITTER, ((1, 2),), 12, 7, cap_compat=True, seed=107),
]}

# one launch of four parameter sets, each with its own rates and initial distribution
MULTI_SET = [
    Scenario("set0", BD, abi.SEG_BINOMIAL, NPLUS_FITTER, ((1, 1), (2, 1)), 6, 6, seed=108),
    Scenario("set1", BD, abi.SEG_BINOMIAL, NMINUS_FITTER, ((2, 1),), 6, 6, seed=108),
    Scenario("set2", BD, abi.SEG_BINOMIAL, (1.0, 1.0, 0.5, 0.5), ((0, 1), (1, 2)), 6, 6, seed=108),
    Scenario("set3", BD, abi.SEG_BINOMIAL, (0.5, 1.5, 0.25, 1.0), ((0, 2), (1, 1)), 6, 6, seed=108),
]


PERTURBATIONS = ("b1 x 1.01", "pick 1 % toward larger k", "split p = 0.502", "uneven adds no N-", "cell stop one late")


def perturbed_law(sc: Scenario, what: str) -> Law:
    """A deliberately wrong law of `sc` for the power self-tests (ScenarioTooLarge where the wrong chain outgrows
    the budget, as a later cell stop can)."""
    if what == "b1 x 1.01":
        b0, b1, d0, d1 = sc.rates
        return enumerate_law(replace(sc, name=sc.name + "/b1x1.01", rates=(b0, float(np.float32(b1 * 1.01)), d0, d1)))
    kw = {"pick 1 % toward larger k": dict(pick_bias=0.01), "split p = 0.502": dict(split_p=0.502),
          "uneven adds no N-": dict(uneven_adds_nminus=False), "cell stop one late": dict(cells_stop_late=1)}[what]
    return enumerate_law(sc, **kw)


# ------------------------------------------------------------------------- runs shared by the CPU and GPU tests
# Both test files build their runs here, so the seeds and sizes are the same: the GPU's philox and reference-draws
# outputs are bit-identical to the oracle's (test_gpu_parity, test_gpu_refdraws), hence the CPU file decides whether
# each seeded GPU assertion passes.

B, R = abi.FLAG_BIN_STORE, abi.FLAG_REFERENCE_DRAWS
INF = float("inf")
STORES = {"rows": (0, 0), "bins32": (B, 32), "bins64": (B, 64), "bins256": (B, 256), "ref": (R, 0)}
SPLIT_KS = [1, 8, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 5000, 32767]
NO_UNEVEN_KS = [1, 2, 3]
YULE_T = math.log(2.0)
# one-event channel and time laws: populations (n-, N+ cells) at which the four propensities under NPLUS_FITTER differ
CHANNEL_POPS = [((0, 3), (1, 1)), ((0, 1), (1, 2), (2, 2)), ((0, 5), (2, 3))]
PICK_INIT = ((1, 3), (2, 2), (70, 4))
# the one-event pick runs 2^22 replicates: at 2^20 a pick weighted 1 % toward the 70-copy cells was rejected at
# p = 2.2e-6 only (a shift of 0.25 % of one proportion, z = 4.7), short of P_MIN / 1000
PICK_REPLICATES = 1 << 22


def _store(store: str, flags: int, kw: dict) -> dict:
    f, k = STORES[store]
    kw = dict(kw)
    kw.setdefault("cell_cap", 16)
    kw.setdefault("hist_bins", 4)
    kw.setdefault("n_replicates", N_REPLICATES)
    kw.setdefault("max_time", INF)
    return dict(flags=f | flags, bin_kmax=k, **kw)


def scenario_spec(sc, store: str, flags: int = 0, **kw) -> "abi.RunSpec":
    """A joint-state scenario (or the list of the multi-set launch) in one of the STORES."""
    f, k = STORES[store]
    if isinstance(sc, Scenario):
        return sc.spec(flags=f | flags, bin_kmax=k, **kw)
    return multi_set_spec(sc, flags=f | flags, bin_kmax=k, **kw)


def channel_spec(i: int, store: str, f32: bool = False, flags: int = 0, **kw) -> "abi.RunSpec":
    flags |= abi.FLAG_TIME_F32 if f32 else 0
    return abi.RunSpec(process=BD, rates=(NPLUS_FITTER,), init=dict(CHANNEL_POPS[i]), max_cells=16, max_iter=1,
                       seed=200 + i, **_store(store, flags, kw))


def check_channel(res, i: int) -> Dict[str, float]:
    """One event from CHANNEL_POPS[i]: the channel against its four propensities, the time against Exp(a0)."""
    init = dict(CHANNEL_POPS[i])
    nm = init.get(0, 0)
    n_plus = sum(c for k, c in init.items() if k > 0)
    b0, b1, d0, d1 = NPLUS_FITTER
    a = np.array([b0 * nm, b1 * n_plus, d0 * nm, d1 * n_plus])
    assert len(set(a.tolist())) == 4
    s = res.summaries
    n = len(s)
    ok = (s["iters"] == 1).all() and (s["stop_reason"] == abi.STOP_MAX_ITER).all() and not s["error"].any()
    return {"one_event": 1.0 if ok else 0.0,
            "channel": chi2_lumped(res.totals[0]["events_by_type"], a / a.sum() * n),
            "time_ks": ks_exp_pvalue(s["time"], float(a.sum())),
            "mean_time": z_pvalue(float(s["time"].mean()), 1.0 / a.sum(), 1.0 / a.sum() ** 2, n)}


def split_reads_hist(k: int) -> bool:
    """The engine takes at most 4096 histogram bins: beyond k = 2047 the split is read off the final rows."""
    return 2 * k + 2 <= 4096


def split_needs_rows(k: int, store: str) -> bool:
    return store in ("rows", "ref") or not split_reads_hist(k)


def split_spec(k: int, store: str, no_uneven: bool = False, flags: int = 0, **kw) -> "abi.RunSpec":
    seg = abi.SEG_BINOMIAL_NO_UNEVEN if no_uneven else abi.SEG_BINOMIAL
    kw.setdefault("hist_bins", 2 * k + 2 if split_reads_hist(k) else 4)  # bins 0 .. 2k of their own
    return abi.RunSpec(process=PB, segregation=seg, rates=((1.0, 1.0, 0.0, 0.0),), init={k: 1}, max_cells=4, max_iter=1,
                       seed=(400 if no_uneven else 300) + SPLIT_KS.index(k) if k in SPLIT_KS else 450 + k,
                       **_store(store, flags, kw))


def check_split(res, k: int, no_uneven: bool = False, ordered_rows: bool = False,
                split_p: float = 0.5) -> Dict[str, float]:
    """One division of one k-copy cell against Binomial(2k, 1/2): folded, from the pooled histogram (any store; k up
    to 2047) or from the sorted final rows (the bin store beyond), and, where the final row keeps the daughters in
    draw order (row store: k1 then 2k - k1), unfolded from the rows."""
    s = res.summaries
    n = len(s)
    ok = (s["iters"] == 1).all() and not s["error"].any() and (s["nplus"] + s["nminus"] == 2).all()
    out = {"one_event": 1.0 if ok else 0.0,
           "uneven": binom_pvalue(int(res.totals[0]["uneven"]), n, 0.0 if no_uneven else 2.0 ** (1 - 2 * k))}
    if split_reads_hist(k):
        out["split_hist"] = split_pvalue_from_hist(res.hist[0], int(s["nminus"].sum()), k, n, no_uneven=no_uneven)
    elif not ordered_rows:
        pair = res.rows[:, :2].astype(np.int64)
        sums_ok = ((s["nplus"] != 2) | (pair.sum(1) == 2 * k)).all()
        out["split_rows_folded"] = split_pvalue(np.where(s["nplus"] == 2, pair.min(1), 0), k, no_uneven=no_uneven,
                                                folded=True) if sums_ok else 0.0
    if ordered_rows:
        k1 = np.where(s["nplus"] == 2, res.rows[:, 0].astype(np.int64), 0)
        out["split_rows"] = split_pvalue(k1, k, no_uneven=no_uneven, p=split_p)
        # the mean of k1 over the even splits: the exact mean and variance of Binomial(2k, p) given 0 < k1 < 2k
        even = s["nplus"] == 2
        j = np.arange(1, 2 * k)
        pmf = stats.binom.pmf(j, 2 * k, split_p)
        pmf /= pmf.sum()
        mean = float((pmf * j).sum())
        var = float((pmf * (j - mean) ** 2).sum())
        out["mean_k1"] = z_pvalue(float(k1[even].mean()), mean, var if k > 1 else 0.0, int(even.sum()))
    return out


def pick_specs(store: str, flags: int = 0, **kw):
    """The one-event pick as PICK_REPLICATES / 2^20 launches of 2^20 replicates (ids continue from launch to launch),
    so that no launch downloads more rows than the other tests do."""
    out = []
    for j in range(PICK_REPLICATES // N_REPLICATES):
        out.append(abi.RunSpec(process=PB, rates=((1.0, 1.0, 0.0, 0.0),), init=dict(PICK_INIT), max_cells=16,
                               max_iter=1, seed=500, first_replicate=j * N_REPLICATES, reps_per_set=PICK_REPLICATES,
                               **_store(store, flags, kw)))
    return out


def picked_counts(res) -> Optional[np.ndarray]:
    """How many replicates of one pick launch picked a 1-, 2- and 70-copy cell (None: an impossible outcome). A
    division doubles the picked cell's copies (k1 + k2 = 2k, or one cell of 2k), so the picked k is the growth of
    the row's sum."""
    s = res.summaries
    n_plus = s["nplus"].astype(np.int64)
    r = res.rows.astype(np.int64)
    r[np.arange(r.shape[1])[None, :] >= n_plus[:, None]] = 0
    picked = r.sum(1) - sum(k * c for k, c in PICK_INIT)
    ks = np.array([k for k, _ in PICK_INIT])
    idx = np.searchsorted(ks, picked)
    if ((idx >= len(ks)) | (ks[np.minimum(idx, len(ks) - 1)] != picked)).any() or (s["iters"] != 1).any():
        return None
    return np.bincount(idx, minlength=len(ks))


def check_pick(counts, pick_bias: float = 0.0) -> Dict[str, float]:
    """The summed picked_counts of the pick launches against cells(1) : cells(2) : cells(70)."""
    if any(c is None for c in counts):
        return {"pick": 0.0}
    obs = np.sum(counts, axis=0)
    wts = np.array([c for _, c in PICK_INIT], dtype=np.float64)
    wts[-1] *= 1.0 + pick_bias  # (a deliberately wrong law for the power tests)
    return {"pick": chi2_lumped(obs, wts / wts.sum() * obs.sum())}


def yule_spec(store: str, f32: bool = False, flags: int = 0, **kw) -> "abi.RunSpec":
    flags |= abi.FLAG_TIME_F32 if f32 else 0
    kw.update(max_time=YULE_T, cell_cap=64)
    return abi.RunSpec(process=PB, rates=((1.0, 1.0, 0.0, 0.0),), init={1: 1}, max_cells=64, seed=600,
                       **_store(store, flags, kw))


def check_yule(res) -> Dict[str, float]:
    s = res.summaries
    ok = (s["stop_reason"] == abi.STOP_MAX_TIME).all() and not s["error"].any() and (s["time"] >= YULE_T).all()
    cells = (s["nminus"] + s["nplus"]).astype(np.int64)
    # one event more than the cells say would be an off-by-one of the stop test: the events are cells - 1
    ok = ok and (s["iters"].astype(np.int64) == cells - 1).all()
    return {"time_stop": 1.0 if ok else 0.0, "cells": yule_stop_pvalue(cells, YULE_T)}


def assert_laws(ps, label):
    worst = min(ps, key=ps.get)
    print(f"LAW {label} | {worst} | {ps[worst]:.3g}")
    bad = {k: v for k, v in ps.items() if not v > P_MIN}
    assert not bad, f"{label}: {bad}"
