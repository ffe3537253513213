"""The host side of the timepoint keep block on the CPU (ecdna-evo_amd/csrc/ssa_keep.hpp): the timepoints T of
a context, the bytes the kept samples take, and every branch of the block's validation.

tests/native/timepoint_keep_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc absent")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("timepoint_keep_check")), "timepoint_keep_check")
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "ecdna-evo_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "timepoint_keep_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-4000:]  # (no sanitizer report)
    return out.stdout.splitlines()


def _want(T, n, m):
    n1 = max(n, 1)
    return [f"cells {T * n1 * m * 2} headers {T * n1 * 8} all {T * n1 * (2 * m + 8)}"]


def test_bytes_of_the_kept_samples(check):
    # the C4 sweep at T = 4 and m = 200: T x n x (2m + 8) bytes, 6.8e9 (arithmetic, not a measurement)
    assert _run(check, "bytes", 4, 4194304, 200) == _want(4, 4194304, 200)
    assert 4 * 4194304 * (2 * 200 + 8) == 6845104128
    assert _run(check, "bytes", 64, (1 << 32) - 1, 4096) == _want(64, (1 << 32) - 1, 4096)  # no overflow of u64
    assert _run(check, "bytes", 3, 0, 64) == ["cells 384 headers 24 all 408"]  # an empty call holds one replicate's
    assert _run(check, "bytes", 1, 7, 1) == _want(1, 7, 1)


def test_every_validation_branch(check):
    assert _run(check, "validate") == ["validate ok"]
