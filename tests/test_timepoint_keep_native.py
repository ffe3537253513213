"""The host side of the timepoint keep block on the CPU (ecdna-evo_amd/csrc/ssa_keep.hpp): the timepoints T of
a context, the bytes the kept samples take, and every branch of the block's validation.

tests/native/timepoint_keep_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return native.build(tmp_path_factory, "timepoint_keep_check")


def _want(T, n, m):
    n1 = max(n, 1)
    return [f"cells {T * n1 * m * 2} headers {T * n1 * 8} all {T * n1 * (2 * m + 8)}"]


def test_bytes_of_the_kept_samples(check):
    # the C4 sweep at T = 4 and m = 200: T x n x (2m + 8) bytes, 6.8e9 (arithmetic, not a measurement)
    assert native.run(check, "bytes", 4, 4194304, 200) == _want(4, 4194304, 200)
    assert 4 * 4194304 * (2 * 200 + 8) == 6845104128
    assert native.run(check, "bytes", 64, (1 << 32) - 1, 4096) == _want(64, (1 << 32) - 1, 4096)  # no overflow of u64
    assert native.run(check, "bytes", 3, 0, 64) == ["cells 384 headers 24 all 408"]  # an empty call holds one replicate's
    assert native.run(check, "bytes", 1, 7, 1) == _want(1, 7, 1)


def test_every_validation_branch(check):
    assert native.run(check, "validate") == ["validate ok"]
