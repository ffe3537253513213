"""The host side of the cohort block on the CPU (ecdna-evo_amd/csrc/ssa_cohort.hpp): the grouping of the targets by
distinct sample size, the LDS plan of the cohort pass at its limits, and every branch of the block's validation.

tests/native/cohort_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native

PASS_LDS_MAX = 65536  # kPassLdsMax

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def cohort_check(tmp_path_factory):
    return native.build(tmp_path_factory, "cohort_check")


def _groups(exe, sizes):
    """[(m, [targets])] and the largest m, as the program printed them."""
    lines = [ln.split() for ln in native.run(exe, "groups", *sizes)]
    assert lines[0][0] == "groups" and lines[0][2] == "max" and int(lines[0][1]) == len(lines) - 1
    return [(int(ln[1]), [int(t) for t in ln[3:]]) for ln in lines[1:]], int(lines[0][3])


def _want(sizes):
    """The grouping restated: distinct sizes in order of first appearance, a group's targets ascending."""
    order = list(dict.fromkeys(sizes))
    return [(m, [t for t, x in enumerate(sizes) if x == m]) for m in order], max(sizes, default=0)


def test_groups_are_the_distinct_sizes_in_order_of_first_appearance(cohort_check):
    cases = [
        (64, 1500, 1, 64, 4096, 65),  # a duplicate
        (300, 5, 300, 5, 5, 300, 7),  # several, interleaved
        (9,) * 64,  # all equal at P = 64: one group
        tuple(range(4096, 4096 - 64, -1)),  # all distinct at P = 64, descending: 64 groups in that order
        (4096,) * 63 + (4095,), (4095,) + (4096,) * 63,
        (1,),
    ]
    for sizes in cases:
        got, top = _groups(cohort_check, sizes)
        assert (got, top) == _want(sizes), sizes
        assert sorted(t for _, ts in got for t in ts) == list(range(len(sizes)))  # every target in exactly one group
    assert _groups(cohort_check, ()) == ([], 0)  # no sample sizes: no groups
    got, _ = _groups(cohort_check, (64, 1500, 1, 64, 4096, 65))
    assert got == [(64, [0, 3]), (1500, [1]), (1, [2]), (4096, [4]), (65, [5])]


def test_lds_plan_stays_within_the_pass_limit(cohort_check):
    lines = native.run(cohort_check, "lds")
    assert lines[0] == "lds ok"
    w = lines[1].split()
    assert w[0] == "limits"
    top = dict(zip(w[1::2], map(int, w[2::2])))
    # 2,048 bins, m = 4096, K = 256: the full and the sample histogram, the prefix sums and a table of 8,192 slots,
    # which also holds the 2,048 f64 of the CDF
    assert top == {"waves": 1, "table_slots": 8192, "scratch_words": 8192,
                   "lds_bytes": (2 * 2048 + 256 + 8192) * 4}
    assert top["lds_bytes"] <= PASS_LDS_MAX


def test_every_validation_branch(cohort_check):
    assert native.run(cohort_check, "validate") == ["validate ok"]
