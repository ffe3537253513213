"""The host side of the sized rescore on the CPU (ecdna-evo_amd/csrc/ssa_thin.hpp; thinning mapping v1): the grouping of
the targets by (measured cells, draw index), the thinning stream's tag, the LDS plan of the thinning pass at its limits,
and every branch of the two calls' validation.

tests/native/thin_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import pytest

from support import native

PASS_LDS_MAX = 65536  # kPassLdsMax

pytestmark = native.needs_hipcc


@pytest.fixture(scope="module")
def thin_check(tmp_path_factory):
    return native.build(tmp_path_factory, "thin_check")


def _groups(exe, keep, pairs, with_draws=True):
    """[((m1, d), [targets])] and the largest m', as the program printed them."""
    words = [f"{m}:{d}" if with_draws else str(m) for m, d in pairs]
    lines = [ln.split() for ln in native.run(exe, "groups", keep, *words)]
    assert lines[0][0] == "groups" and lines[0][2] == "max_mp" and int(lines[0][1]) == len(lines) - 1
    return [((int(ln[1]), int(ln[3])), [int(t) for t in ln[5:]]) for ln in lines[1:]], int(lines[0][3])


def _want(keep, pairs):
    """The grouping restated: distinct (m1, d) in order of first appearance, a group's targets ascending; the largest
    m' = min(m1, keep_cells - m1)."""
    order = list(dict.fromkeys(pairs))
    return ([(k, [t for t, x in enumerate(pairs) if x == k]) for k in order],
            max((min(m, keep - m) for m, _ in pairs), default=0))


def test_groups_are_the_distinct_pairs_in_order_of_first_appearance(thin_check):
    cases = [
        (199, ((199, 0), (90, 0), (130, 0), (1, 3), (198, 0), (60, 63))),
        (200, ((100, 0), (100, 1), (100, 0), (80, 1), (100, 1), (80, 0), (80, 1))),  # duplicates, interleaved
        (4096, ((9, 5),) * 64),  # all equal at P = 64: one group
        (4096, tuple((4096 - i, 0) for i in range(64))),  # all distinct sizes at P = 64: 64 groups in that order
        (200, tuple((100, d) for d in range(64))),  # all distinct draws at P = 64
        (200, tuple((100 + (i % 8), i // 8) for i in range(64))),  # all distinct pairs at P = 64
        (4096, ((2048, 0),)), (4096, ((4096, 63),)), (1, ((1, 0),)),
    ]
    for keep, pairs in cases:
        got, top = _groups(thin_check, keep, pairs)
        assert (got, top) == _want(keep, pairs), (keep, pairs)
        assert sorted(t for _, ts in got for t in ts) == list(range(len(pairs)))  # every target in exactly one group
        assert top <= keep // 2
    assert _groups(thin_check, 200, ()) == ([], 0)  # no sizes: no groups
    # no draws: every d is 0
    got, top = _groups(thin_check, 200, ((100, 7), (100, 9), (30, 1)), with_draws=False)
    assert (got, top) == ([((100, 0), [0, 1]), ((30, 0), [2])], 100)
    got, top = _groups(thin_check, 199, cases[0][1])
    assert got == [((199, 0), [0]), ((90, 0), [1]), ((130, 0), [2]), ((1, 3), [3]), ((198, 0), [4]), ((60, 63), [5])]
    assert top == 90


def test_tag_fields_stay_disjoint(thin_check):
    lines = native.run(thin_check, "tag")
    assert lines[0] == "tag ok"
    # s = 63, d = 63, t = 1023: tag | snapshot field | thinning flag | draw | block
    assert lines[1] == "top 0x%08x" % (0xC0000000 | (64 << 16) | 0x20000000 | (63 << 10) | 1023)


def test_lds_plan_stays_within_the_pass_limit(thin_check):
    lines = native.run(thin_check, "lds")
    assert lines[0] == "lds ok"
    w = lines[1].split()
    assert w[0] == "limits"
    top = dict(zip(w[1::2], map(int, w[2::2])))
    # 2,048 bins, keep_cells = 4096: m' <= 2,048, a table of 4,096 slots, which also holds the 2,048 f64 of the CDF,
    # beside the full and the thinned histogram: 32 KiB per wave, two waves
    assert top == {"max_mp": 2048, "waves": 2, "table_slots": 4096, "scratch_words": 4096,
                   "lds_bytes": 2 * (2 * 2048 + 4096) * 4}
    assert top["lds_bytes"] <= PASS_LDS_MAX


def test_every_validation_branch(thin_check):
    assert native.run(thin_check, "validate") == ["validate ok"]
