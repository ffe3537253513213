"""The host side of the pooling over thinning draws on the CPU (ecdna-evo_amd/csrc/ssa_pool_draws.hpp; thinned pooling
mapping v1): every branch of the call's validation, the verdict's and the pooling's grouping of the targets, the LDS
plan at its limits, the byte counts, and the launches' check of the group tables (ssa_launch.h grouping_ok).

tests/native/pool_draws_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native
from support.native import _want_keep, _want_timepoints

PASS_LDS_MAX = 65536  # kPassLdsMax

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return native.build(tmp_path_factory, "pool_draws_check")


def _grouping(lines, name):
    """(slices, slice mask, max m', [(first group, end group)] per slice, [(m1, [targets])] per group) of one grouping as
    printed, and the lines after it."""
    head = lines[0]
    assert head[0] == name and head[1::2] == ["slices", "mask", "groups", "max_mp"]
    n_slices, n_groups = int(head[2]), int(head[6])
    slices = [(int(ln[3]), int(ln[4])) for ln in lines[1:1 + n_slices]]
    groups = [(int(ln[1]), [int(t) for t in ln[3:]]) for ln in lines[1 + n_slices:1 + n_slices + n_groups]]
    return (n_slices, int(head[4], 16), int(head[8]), slices, groups), lines[1 + n_slices + n_groups:]


def _plan(exe, keep, timepoints, mask, sizes):
    """(the verdict's grouping, the pooling's, the max m' the LDS plan is sized for)."""
    lines = [ln.split() for ln in native.run(exe, "plan", keep, int(timepoints), "%x" % mask, *sizes)]
    verdict, rest = _grouping(lines, "verdict")
    pool, rest = _grouping(rest, "pool")
    assert len(rest) == 1 and rest[0][:2] == ["lds", "max_mp"]
    return verdict, pool, int(rest[0][2])


def test_the_keep_store_pools_held_out_targets_too(check):
    cases = [
        (199, 0, (90, 130, 90)),
        (199, 0b101, (90, 130, 90)),                # the target in between is held out of the verdict, not of the pools
        (199, 0b010, (90, 130, 90)),
        (200, 0b1010101, (100, 80, 100, 80, 100, 7, 80)),
        (4096, 1 << 63, tuple(4096 - i for i in range(64))),
        (4096, 0, (9,) * 64),
        (4096, 0, (2048,)), (4096, 0, (4096,)), (1, 0, (1,)),
    ]
    for keep, mask, sizes in cases:
        verdict, pool, lds_mp = _plan(check, keep, False, mask, sizes)
        assert verdict == _want_keep(keep, mask, sizes), (keep, mask, sizes)
        assert pool == _want_keep(keep, 0, sizes), (keep, mask, sizes)  # the pooling grouping: mask 0
        assert sorted(t for _, ts in pool[4] for t in ts) == list(range(len(sizes)))  # every slot is in one group
        assert lds_mp == pool[2] >= verdict[2]
    verdict, pool, lds_mp = _plan(check, 199, False, 0b101, (90, 130, 90))
    assert verdict == (1, 1, 90, [(0, 1)], [(90, [0, 2])])
    assert pool == (1, 1, 90, [(0, 2)], [(90, [0, 2]), (130, [1])])
    verdict, pool, lds_mp = _plan(check, 200, False, 0b001, (7, 100))  # the held-out target sizes the table
    assert verdict[2] == 7 and pool[2] == lds_mp == 100


def test_the_timepoint_store_pools_one_group_per_slice_whatever_the_mask(check):
    cases = [
        (50, 0, (20, 50, 35)), (50, 0b101, (20, 50, 35)), (50, 0b010, (20, 50, 35)), (50, 0b100, (20, 50, 35)),
        (100, 0, (40, 40)), (100, 0b10, (40, 40)),
        (4096, 1 << 63 | 1, tuple(1 + 64 * i for i in range(64))),
    ]
    for keep, mask, sizes in cases:
        verdict, pool, lds_mp = _plan(check, keep, True, mask, sizes)
        assert verdict == _want_timepoints(keep, mask, sizes), (keep, mask, sizes)
        assert pool == _want_timepoints(keep, 0, sizes), (keep, mask, sizes)
        T = len(sizes)
        assert pool[3] == [(t, t + 1) for t in range(T)] and pool[4] == [(sizes[t], [t]) for t in range(T)]
        assert lds_mp == pool[2]
    verdict, pool, _ = _plan(check, 50, True, 0b101, (20, 50, 35))
    assert verdict == (3, 0b101, 20, [(0, 1), (1, 1), (1, 2)], [(20, [0]), (35, [2])])
    assert pool == (3, 0b111, 20, [(0, 1), (1, 2), (2, 3)], [(20, [0]), (50, [1]), (35, [2])])


def test_lds_plan_stays_within_the_pass_limit(check):
    lines = native.run(check, "lds")
    assert lines[0] == "lds ok"
    got = {}
    for ln in lines[1:]:
        w = ln.split()
        d = dict(zip(w[0::2], map(int, w[1::2])))
        got[(d.pop("bins"), d.pop("keep"))] = d
    # thin's plan plus the words of one [bins] u32 array per wave that do not fit behind the table; 2,048 bins beside
    # keep_cells = 4096 and m1 = 2048: 2 * 2048 + 4096 scratch + 2048 words = 40 KiB, one wave per workgroup
    assert got[(2048, 4096)] == {"max_mp": 2048, "waves": 1, "table_slots": 4096, "scratch_words": 4096,
                                 "lds_bytes": (2 * 2048 + 4096 + 2048) * 4}
    assert got[(2048, 4096)]["lds_bytes"] == 40 * 1024 <= PASS_LDS_MAX
    # no table at keep_cells = 1 (every sample is scored whole): the accumulator fits where the CDF lies, thin's plan
    assert got[(2048, 1)] == {"max_mp": 0, "waves": 2, "table_slots": 0, "scratch_words": 4096,
                              "lds_bytes": 2 * (2 * 2048 + 4096) * 4}
    # (four waves of 4 + 4,096 + 2 words would take 96 bytes more than 64 KiB)
    assert got[(2, 4096)] == {"max_mp": 2048, "waves": 2, "table_slots": 4096, "scratch_words": 4096,
                              "lds_bytes": 2 * (2 * 2 + 4096 + 2) * 4}
    assert got[(2, 1)] == {"max_mp": 0, "waves": 4, "table_slots": 0, "scratch_words": 4,
                           "lds_bytes": 4 * (2 * 2 + 4) * 4}
    assert all(d["lds_bytes"] <= PASS_LDS_MAX for d in got.values())


def test_byte_counts(check):
    lines = native.run(check, "bytes")
    got = [dict(zip(w[0::2], map(int, w[1::2]))) for w in (ln.split() for ln in lines)]
    # (n_targets + n_slices) x n_param_sets x hist_bins x 8 bytes
    assert got[0] == {"thinned": 2 * 1024 * 1025, "kept": 1024 * 1025, "pooled": (2 + 1) * 1024 * 1025 * 8,
                      "cdf": 2 * 1025 * 8, "scalars": 2 * 3 * 8}
    assert got[1] == {"thinned": 4 * 3 * 33, "kept": 4 * 3 * 33, "pooled": (4 + 4) * 3 * 33 * 8, "cdf": 4 * 33 * 8,
                      "scalars": 4 * 3 * 8}


def test_every_validation_branch(check):
    assert native.run(check, "validate") == ["validate ok"]


def test_the_launch_check_takes_every_planned_grouping_and_refuses_each_broken_table(check):
    lines = native.run(check, "grouping")
    # 8 bins x 8 keep sizes x 2 stores x 3 masks, and per case the verdict's, the pooling's and accept_draws' own plan
    assert lines[0] == "accepted %d" % (8 * 8 * 2 * 3 * 3)
    # one refusal per clause of the conditions launch_accept_draws and launch_pool_draws had spelled out
    assert lines[1:] == ["refused " + what for what in (
        "a decreasing group_offset", "a decreasing slice_group", "slice_group[n_slices] != n_groups",
        "a target index >= n_targets", "group_m of 0", "group_m of m + 1", "n_groups of 0", "n_groups of n_targets + 1",
        "slice_group[0] != 0", "group_offset[0] != 0", "group_offset[n_groups] > n_targets",
        "no slice", "65 slices", "65 targets")]
