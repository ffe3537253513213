"""The host side of the acceptance over repeated thinnings on the CPU (ecdna-evo_amd/csrc/ssa_accept_draws.hpp; thinned
acceptance mapping v1): every branch of the call's validation, the per-slice grouping of the participating targets, the
LDS plan at its limits and the byte counts.

tests/native/accept_draws_check.cpp is a stand-alone program, built for the host alone with the address and
undefined-behaviour sanitizers (any report ends it with an error); it is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_LDS_MAX = 65536  # kPassLdsMax

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc absent")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("accept_draws_check")), "accept_draws_check")
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "ecdna-evo_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "accept_draws_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-4000:]  # (no sanitizer report)
    return out.stdout.splitlines()


def _plan(exe, keep, timepoints, mask, sizes):
    """(slices, slice mask, max m', [(first group, end group)] per slice, [(m1, [targets])] per group) as printed."""
    lines = [ln.split() for ln in _run(exe, "plan", keep, int(timepoints), "%x" % mask, *sizes)]
    head = lines[0]
    assert head[0::2] == ["slices", "mask", "groups", "max_mp"]
    n_slices, n_groups = int(head[1]), int(head[5])
    assert len(lines) == 1 + n_slices + n_groups
    slices = [(int(ln[3]), int(ln[4])) for ln in lines[1:1 + n_slices]]
    groups = [(int(ln[1]), [int(t) for t in ln[3:]]) for ln in lines[1 + n_slices:]]
    return n_slices, int(head[3], 16), int(head[7]), slices, groups


def _want_keep(keep, mask, sizes):
    """The keep store restated: one slice; the participating targets by distinct m1 in order of first appearance."""
    take = [p for p in range(len(sizes)) if mask == 0 or (mask >> p) & 1]
    order = list(dict.fromkeys(sizes[p] for p in take))
    groups = [(m, [p for p in take if sizes[p] == m]) for m in order]
    return 1, 1, max(min(m, keep - m) for m in order), [(0, len(groups))], groups


def _want_timepoints(keep, mask, sizes):
    """The timepoint store restated: slice t takes part when the mask names it, with one group of target t."""
    T = len(sizes)
    full = mask if mask else (1 << T) - 1
    take = [t for t in range(T) if (full >> t) & 1]
    slices, at = [], 0
    for t in range(T):
        slices.append((at, at + (t in take)))
        at += t in take
    return T, full, max(min(sizes[t], keep - sizes[t]) for t in take), slices, [(sizes[t], [t]) for t in take]


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
    lines = _run(check, "lds")
    assert lines[0] == "lds ok"
    w = lines[1].split()
    assert w[0] == "limits"
    top = dict(zip(w[1::2], map(int, w[2::2])))
    # 2,048 bins, keep_cells = 4096, m1 = 2048: the thinning pass's plan — 32 KiB per wave, two waves, 64 KiB
    assert top == {"max_mp": 2048, "waves": 2, "table_slots": 4096, "scratch_words": 4096,
                   "lds_bytes": 2 * (2 * 2048 + 4096) * 4}
    assert top["lds_bytes"] <= PASS_LDS_MAX


def test_byte_counts(check):
    w = _run(check, "bytes")[0].split()
    got = dict(zip(w[0::2], map(int, w[1::2])))
    n = 4194304
    # the C4 sweep: the call keeps n x Q bytes where the loop's 64 draws take 64 records of 64 bytes per replicate
    assert got == {"passes": n * 8, "sums": 8 * 1024 * 8, "cdf": 2 * 1025 * 8, "scalars": 2 * 3 * 8,
                   "loop": 64 * n * 64}
    assert got["loop"] == 17179869184


def test_every_validation_branch(check):
    assert _run(check, "validate") == ["validate ok"]
