"""The host side of the select over thinning draws on the CPU (ecdna-evo_amd/csrc/ssa_select_draws.hpp; thinned select
mapping v1): every branch of the call's validation with its message — the block of ecdna_ssa_ctx_accept_draws without
threshold rows, the 32-bit bound of the keys, the rank rules and the rules of a digit pass — that accept_draws::invalid
answers as before, the byte counts, and the comparison "same block as the cached keys".

tests/native/select_draws_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return native.build(tmp_path_factory, "select_draws_check")


def test_every_validation_branch(check):
    assert native.run(check, "validate") == ["validate ok"]


def test_byte_counts_and_the_bound_of_the_keys(check):
    got = [dict(zip(w[0::2], map(int, w[1::2]))) for w in (ln.split() for ln in native.run(check, "bytes"))]
    hist = 4 * 32 * 256 * 8  # one pass: [4][32 groups][256] u64
    small = {"hist": hist, "cdf": 4 * 1025 * 8, "scalars": 4 * 3 * 8}
    # 32 bytes per (replicate, draw): 2.1 GB at the keep shape of the measurement
    assert got[0] == dict(n=1 << 20, draws=64, n_keys=1 << 26, keys=32 << 26, taken=1, **small)
    assert got[0]["keys"] == 2147483648
    assert got[1] == dict(n=131072, draws=64, n_keys=1 << 23, keys=32 << 23, taken=1, **small)
    assert got[2] == dict(n=258, draws=3, n_keys=774, keys=774 * 32, taken=1, **small)
    # 2^26 replicates on 64 draws are 2^32 keys: refused, one replicate fewer is taken
    assert got[3] == dict(n=1 << 26, draws=64, n_keys=1 << 32, keys=32 << 32, taken=0, **small)
    assert got[4] == dict(n=(1 << 26) - 1, draws=64, n_keys=(1 << 32) - 64, keys=32 * ((1 << 32) - 64), taken=1, **small)


def test_the_same_block_comparison(check):
    assert native.run(check, "same") == ["same ok"]
