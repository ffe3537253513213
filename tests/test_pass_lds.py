"""The sampling passes' LDS plan on the CPU: how many waves a workgroup of ssa_subsample, ssa_passage and ssa_snapstats
gets, how many bytes of dynamic LDS, and whether ssa_snapstats keeps the workgroup's sample histogram in LDS
(ecdna-evo_amd/csrc/ssa_launch.h), exported for this test as ecdna_dev_pass_lds (not part of the C ABI). The three
formulas are restated here as they stood when each pass had its own function: 1, 2 or 4 waves, the most that keep the
workgroup within 64 KiB."""
import itertools

import pytest

from support.pass_lds import (BAG_K, BINS, LDS_MAX, M, PASSAGE, SNAPSTATS, SUBSAMPLE, passage_plan,  # noqa: F401
                              plan, snapstats_plan, subsample_plan)  # (plan: fixture)


@pytest.mark.parametrize("which,restated", [(SUBSAMPLE, subsample_plan), (PASSAGE, passage_plan)],
                         ids=["subsample", "passage"])
def test_per_replicate_passes(plan, which, restated):
    for bins, bag_k, m in itertools.product(BINS, BAG_K, M):
        got = plan(which, bins, bag_k, m)
        assert got == restated(bins, bag_k, m), (bins, bag_k, m)
        assert got[0] in (1, 2, 4) and got[1] <= LDS_MAX, (bins, bag_k, m)


def test_snapstats(plan):
    for bins, bag_k, m in itertools.product(BINS, BAG_K, (0,) + M):
        got = plan(SNAPSTATS, bins, bag_k, m)  # (the pass reads expanded rows: bag_k does not enter)
        assert got == snapstats_plan(bins, m), (bins, m)
        assert got[0] in (1, 2, 4) and got[1] <= LDS_MAX, (bins, m)
        if m == 0:
            assert got[2] == 0


def test_the_limits_take_one_wave(plan):
    """2,048 bins beside m = 4096: one wave per workgroup in every pass, the snapshot samples' histogram in global memory."""
    assert plan(SUBSAMPLE, 2048, 256, 4096) == (1, 2048 * 8 + (2048 + 256 + 8192) * 4, 0)
    assert plan(PASSAGE, 2048, 256, 4096) == (1, (2048 + 256 + 8192 + 2048) * 4, 0)
    assert plan(SNAPSTATS, 2048, 0, 4096) == (1, 2048 * 8 + (2048 + 8192) * 4, 0)
    assert plan(SNAPSTATS, 257, 0, 500) == (4, 2 * 257 * 8 + 4 * (257 + 1024) * 4, 1)
