"""The LDS plan of the snapshot keep pass on the CPU (ecdna-evo_amd/csrc/ssa_launch.h, through ecdna_dev_pass_lds, which
is not part of the C ABI): selector 6. The pass is ssa_passage's KEEP = 2 instance over a population that is a snapshot
row only, so it takes the passage pass's plan with bag_k = 0: no workgroup histogram; per wave the histogram and the
table of drawn positions (u32) and the kept cells while they are sorted (u16); 1, 2 or 4 waves, the most that keep the
workgroup within 64 KiB. The selectors 0 .. 5 keep their meaning (tests/test_pass_lds.py, tests/test_pass_lds_keep.py)."""
import itertools
from support.pass_lds import LDS_MAX, PASSAGE, passage_plan, plan, sort_slots, table_slots  # noqa: F401 (plan: fixture)


KEEP_SNAPSHOTS = 6
BINS = (2, 257, 2048)
M = (1, 64, 65, 4096)


def test_snapshot_keep_pass(plan):
    for bins, m in itertools.product(BINS, M):
        got = plan(KEEP_SNAPSHOTS, bins, 0, m)
        per_wave = (bins + table_slots(m) + sort_slots(m) // 2) * 4
        waves = next(nw for nw in (4, 2, 1) if nw * per_wave <= LDS_MAX or nw == 1)
        assert got == (waves, waves * per_wave, 0), (bins, m)
        assert got == passage_plan(bins, 0, m) == plan(PASSAGE, bins, 0, m), (bins, m)
        assert got[0] in (1, 2, 4) and got[1] <= 65536, (bins, m)  # never above 65,536
        for bag_k in (32, 64, 256):  # the populations are rows: the store's K does not enter
            assert plan(KEEP_SNAPSHOTS, bins, bag_k, m) == got, (bins, bag_k, m)


def test_the_limit_takes_one_wave(plan):
    """2,048 bins beside m = 4096: 8 + 32 + 8 KiB, one wave per workgroup."""
    assert plan(KEEP_SNAPSHOTS, 2048, 0, 4096) == (1, 8192 + 32768 + 8192, 0)
    assert plan(KEEP_SNAPSHOTS, 257, 0, 64) == (4, 4 * (257 + 128 + 32) * 4, 0)
    assert plan(KEEP_SNAPSHOTS, 2, 0, 1) == (4, 4 * (2 + 2 + 32) * 4, 0)
