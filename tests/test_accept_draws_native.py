"""The host side of the acceptance over repeated thinnings on the CPU (ecdna-evo_amd/csrc/ssa_accept_draws.hpp; thinned
acceptance mapping v1): every branch of the call's validation, the per-slice grouping of the participating targets, the
LDS plan at its limits and the byte counts.

tests/native/accept_draws_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native
from support.native import _want_keep, _want_timepoints

PASS_LDS_MAX = 65536  # kPassLdsMax

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return native.build(tmp_path_factory, "accept_draws_check")


def _plan(exe, keep, timepoints, mask, sizes):
    """(slices, slice mask, max m', [(first group, end group)] per slice, [(m1, [targets])] per group) as printed."""
    lines = [ln.split() for ln in native.run(exe, "plan", keep, int(timepoints), "%x" % mask, *sizes)]
    head = lines[0]
    assert head[0::2] == ["slices", "mask", "groups", "max_mp"]
    n_slices, n_groups = int(head[1]), int(head[5])
    assert len(lines) == 1 + n_slices + n_groups
    slices = [(int(ln[3]), int(ln[4])) for ln in lines[1:1 + n_slices]]
    groups = [(int(ln[1]), [int(t) for t in ln[3:]]) for ln in lines[1 + n_slices:]]
    return n_slices, int(head[3], 16), int(head[7]), slices, groups


def test_the_keep_store_groups_the_participating_targets(check):
    cases = [
        (199, 0, (90, 130, 90)),                    # a shared sample
        (199, 0b101, (90, 130, 90)),                # the target in between is left out: one group, no 130
        (199, 0b010, (90, 130, 90)),
        (200, 0, (100, 80, 100, 80, 100, 7, 80)),   # duplicates, interleaved
        (200, 0b1010101, (100, 80, 100, 80, 100, 7, 80)),
        (4096, 0, (9,) * 64),                       # all equal at P = 64: one group
        (4096, 0, tuple(4096 - i for i in range(64))),  # all distinct at P = 64: 64 groups in that order
        (4096, 1 << 63, tuple(4096 - i for i in range(64))),
        (4096, 0, (2048,)), (4096, 0, (4096,)), (1, 0, (1,)),
    ]
    for keep, mask, sizes in cases:
        got = _plan(check, keep, False, mask, sizes)
        assert got == _want_keep(keep, mask, sizes), (keep, mask, sizes)
        assert got[2] <= keep // 2
    assert _plan(check, 199, False, 0b101, (90, 130, 90)) == (1, 1, 90, [(0, 1)], [(90, [0, 2])])
    assert _plan(check, 199, False, 0, (90, 130, 90))[2:] == (90, [(0, 2)], [(90, [0, 2]), (130, [1])])


def test_the_timepoint_store_has_one_group_per_participating_slice(check):
    cases = [
        (50, 0, (20, 50, 35)), (50, 0b101, (20, 50, 35)), (50, 0b010, (20, 50, 35)), (50, 0b100, (20, 50, 35)),
        (100, 0, (40, 40)), (100, 0b10, (40, 40)),
        (4096, 0, tuple(1 + 64 * i for i in range(64))), (4096, 1 << 63 | 1, tuple(1 + 64 * i for i in range(64))),
    ]
    for keep, mask, sizes in cases:
        assert _plan(check, keep, True, mask, sizes) == _want_timepoints(keep, mask, sizes), (keep, mask, sizes)
    # equal sizes in different slices are different samples: never one group
    assert _plan(check, 100, True, 0, (40, 40)) == (2, 0b11, 40, [(0, 1), (1, 2)], [(40, [0]), (40, [1])])
    assert _plan(check, 50, True, 0b101, (20, 50, 35)) == (3, 0b101, 20, [(0, 1), (1, 1), (1, 2)], [(20, [0]), (35, [2])])


def test_lds_plan_stays_within_the_pass_limit(check):
    lines = native.run(check, "lds")
    assert lines[0] == "lds ok"
    w = lines[1].split()
    assert w[0] == "limits"
    top = dict(zip(w[1::2], map(int, w[2::2])))
    # 2,048 bins, keep_cells = 4096, m1 = 2048: the thinning pass's plan — 32 KiB per wave, two waves, 64 KiB
    assert top == {"max_mp": 2048, "waves": 2, "table_slots": 4096, "scratch_words": 4096,
                   "lds_bytes": 2 * (2 * 2048 + 4096) * 4}
    assert top["lds_bytes"] <= PASS_LDS_MAX


def test_byte_counts(check):
    w = native.run(check, "bytes")[0].split()
    got = dict(zip(w[0::2], map(int, w[1::2])))
    n = 4194304
    # the C4 sweep: the call keeps n x Q bytes where the loop's 64 draws take 64 records of 64 bytes per replicate
    assert got == {"passes": n * 8, "sums": 8 * 1024 * 8, "cdf": 2 * 1025 * 8, "scalars": 2 * 3 * 8,
                   "loop": 64 * n * 64}
    assert got["loop"] == 17179869184


def test_every_validation_branch(check):
    assert native.run(check, "validate") == ["validate ok"]
