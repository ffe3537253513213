"""The host side of ecdna_ssa_ctx_select on the CPU (ecdna-evo_amd/csrc/ssa_select.hpp): the key map — the function the
kernels of ssa_select.hip call, NaN branch included, which no run reaches — and the driver ssa_api_passes.cpp calls
(select::run: the rank walk over the passes' histograms and the four outputs), against the numpy restatement
(tests/select_law.py), bit for bit.

tests/native/select_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import subprocess

import numpy as np
import pytest

import select_law as sl
from support import native

INF, NAN = np.inf, np.nan

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def select_check(tmp_path_factory):
    return native.build(tmp_path_factory, "select_check")


def _run(exe, values, ranks=None, fractions=None):
    """values: [4][M] f64. Returns select_law.Selected as the program printed it."""
    head = "ranks " + " ".join(str(int(k)) for k in ranks) if ranks is not None else \
        "fractions " + " ".join(repr(float(f)) for f in fractions)
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    text = head + "\n" + "".join("bits " + " ".join(f"{int(b):016x}" for b in row) + "\n" for row in bits)
    lines = [ln.split() for ln in native.run(exe, stdin=text)]
    assert [ln[0] for ln in lines] == ["population", "ranks"] + ["values", "counts"] * 4
    vals = np.array([[int(w, 16) for w in ln[1:]] for ln in lines[2::2]], dtype=np.uint64).view(np.float64)
    counts = np.array([[int(w) for w in ln[1:]] for ln in lines[3::2]], dtype=np.uint64)
    return sl.Selected(int(lines[0][1]), np.array([int(w) for w in lines[1][1:]], dtype=np.uint64), vals, counts)


def _same(got, want):
    assert got.population == want.population
    np.testing.assert_array_equal(got.ranks, want.ranks)
    np.testing.assert_array_equal(got.values.view(np.uint64), want.values.view(np.uint64))
    np.testing.assert_array_equal(got.counts_le, want.counts_le)


def _values(M=700, seed=3):
    rng = np.random.default_rng(seed)
    v = np.zeros((4, M))
    v[0] = np.minimum(1.0, rng.integers(0, 60, M) / 40.0)  # ties, many exactly 1.0
    v[1] = rng.random(M) * 10.0 ** rng.integers(-300, 300, M)  # every byte of the key varies
    v[1, :6] = [NAN, -NAN, INF, -0.0, 0.0, 5e-324]
    v[2] = rng.random(M)
    v[3] = 0.375  # one value: every rank ties
    return v


def test_key_map_on_the_edge_doubles(select_check):
    out = subprocess.run([select_check, "edges"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "" and out.stdout.strip() == "edges ok", out.stderr[-4000:]


def test_walk_gives_the_restatements_order_statistics(select_check):
    v = _values()
    M = v.shape[1]
    ranks = [1, 1, 2, 3, 5, M // 10, M // 2, M // 2, M - 2, M - 1, M, M + 1, 2 ** 64 - 1]
    ranks += [int(k) for k in np.linspace(4, M - 4, 32 - len(ranks))]
    want = sl.select_keys(sl.keys_of(v), ranks=ranks)
    assert np.isnan(want.values[1]).any() and (want.values[1] == INF).any()  # the NaNs sort above +inf
    assert (want.counts_le[0] > want.ranks).any() and np.all(want.counts_le[3][want.ranks <= M] == M)
    _same(_run(select_check, v, ranks=ranks), want)


def test_walk_takes_fractions_and_small_populations(select_check):
    v = _values()
    fr = [1e-9, 0.01, 0.5, 1.0]
    _same(_run(select_check, v, fractions=fr), sl.select_keys(sl.keys_of(v), fractions=fr))
    for M in (0, 1, 2):
        _same(_run(select_check, v[:, :M], ranks=[1, 2, 3]), sl.select_keys(sl.keys_of(v[:, :M]), ranks=[1, 2, 3]))
        _same(_run(select_check, v[:, :M], fractions=[0.5, 1.0]), sl.select_keys(sl.keys_of(v[:, :M]), fractions=[0.5, 1.0]))
