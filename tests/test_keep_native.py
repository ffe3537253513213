"""The host side of the keep block on the CPU (ecdna-evo_amd/csrc/ssa_keep.hpp): the map from a replicate's global id
to its index in the call (ecdna_ssa_ctx_download_kept), the bytes the kept samples take, and every branch of the block's
validation.

tests/native/keep_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def keep_check(tmp_path_factory):
    return native.build(tmp_path_factory, "keep_check")


def _want(first, stride, n, rid):
    """The index restated: the call's replicates are first + i * stride, i < n."""
    d = rid - first
    return str(d // stride) if d >= 0 and d % stride == 0 and d // stride < n else "no"


def test_ids_map_to_their_index_in_the_call(keep_check):
    top = (1 << 64) - 1
    cases = [
        (0, 1, 600, [0, 1, 599, 600, 601, top]),
        (1, 2, 300, [0, 1, 2, 3, 599, 600, 601]),  # the odd shard of two: even ids are off the stride
        (7, 5, 3, [6, 7, 8, 12, 17, 22]),  # before the first, on and off the stride, one past the last
        (top - 4, 2, 3, [top - 4, top - 3, top - 2, top - 1, top, 0]),  # ids at the top of u64
        (5, 3, 0, [5, 8]),  # an empty call has no replicate
        (10, 1, 1, [9, 10, 11]),
    ]
    for first, stride, n, ids in cases:
        got = native.run(keep_check, "index", first, stride, n, *ids)
        assert got == [_want(first, stride, n, r) for r in ids], (first, stride, n)
    assert native.run(keep_check, "index", 1, 2, 300, 1, 3, 599) == ["0", "1", "299"]
    # (the ABI reads a stride of 0 as 1 before it asks; the map itself takes no id under a stride of 0)
    assert native.run(keep_check, "index", 0, 0, 5, 0, 3) == ["no", "no"]


def test_bytes_of_the_kept_samples(keep_check):
    # the C4 sweep at m = 200: n x m x 2 bytes of cells (1.7 GB) and 8 bytes of header per replicate
    assert native.run(keep_check, "bytes", 4194304, 200) == [f"cells {4194304 * 200 * 2} headers {4194304 * 8}"]
    assert native.run(keep_check, "bytes", (1 << 32) - 1, 4096) == [f"cells {((1 << 32) - 1) * 8192} headers {((1 << 32) - 1) * 8}"]
    assert native.run(keep_check, "bytes", 0, 64) == ["cells 128 headers 8"]  # an empty call still holds one replicate's


def test_every_validation_branch(keep_check):
    assert native.run(keep_check, "validate") == ["validate ok"]
