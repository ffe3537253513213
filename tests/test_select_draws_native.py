"""The host side of the select over thinning draws on the CPU (ecdna-evo_amd/csrc/ssa_select_draws.hpp; thinned select
mapping v1): every branch of the call's validation with its message — the block of ecdna_ssa_ctx_accept_draws without
threshold rows, the 32-bit bound of the keys, the rank rules and the rules of a digit pass — that accept_draws::invalid
answers as before, the byte counts, and the comparison "same block as the cached keys".

tests/native/select_draws_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc absent")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("select_draws_check")), "select_draws_check")
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "ecdna-evo_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "select_draws_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-4000:]  # (no sanitizer report)
    return out.stdout.splitlines()


def test_every_validation_branch(check):
    assert _run(check, "validate") == ["validate ok"]


def test_byte_counts_and_the_bound_of_the_keys(check):
    got = [dict(zip(w[0::2], map(int, w[1::2]))) for w in (ln.split() for ln in _run(check, "bytes"))]
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
    assert _run(check, "same") == ["same ok"]
