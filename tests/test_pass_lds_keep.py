"""The LDS plan of the keep block's passes on the CPU (ecdna-evo_amd/csrc/ssa_launch.h, through ecdna_dev_pass_lds, which
is not part of the C ABI): the keep pass (selector 3), ssa_rescore (4) and ssa_pool_accepted (5), over the grid of bins,
K and m of tests/test_pass_lds.py. The formulas are restated here:
 - the keep pass is ssa_passage's KEEP instance and takes the passage pass's plan: no workgroup histogram; per wave the
   histogram, the prefix sums and the table of drawn positions (u32) and the kept cells while they are sorted (u16);
 - ssa_rescore: per wave the sample's histogram (u32 per bin) and its CDF (f64 per bin), 1, 2 or 4 waves;
 - ssa_pool_accepted: one u64 histogram per workgroup of four waves.
The selectors 0 .. 2 keep their meaning (tests/test_pass_lds.py)."""
import itertools
from support.pass_lds import BAG_K, BINS, LDS_MAX, M, PASSAGE, passage_plan, plan, waves_within  # noqa: F401 (plan: fixture)


KEEP, RESCORE, POOL = 3, 4, 5


def rescore_plan(bins):
    return waves_within(lambda nw: nw * (bins * 4 + bins * 8)) + (0,)


def pool_plan(bins):
    return 4, bins * 8, 0


def test_keep_pass(plan):
    for bins, bag_k, m in itertools.product(BINS, BAG_K, M):
        got = plan(KEEP, bins, bag_k, m)
        assert got == passage_plan(bins, bag_k, m) == plan(PASSAGE, bins, bag_k, m), (bins, bag_k, m)
        assert got[0] in (1, 2, 4) and got[1] <= LDS_MAX, (bins, bag_k, m)


def test_rescore_and_pool(plan):
    for bins, bag_k, m in itertools.product(BINS, BAG_K, (0,) + M):  # (neither depends on K or m)
        got = plan(RESCORE, bins, bag_k, m)
        assert got == rescore_plan(bins), (bins, bag_k, m)
        assert got[0] in (1, 2, 4) and got[1] <= LDS_MAX
        assert plan(POOL, bins, bag_k, m) == pool_plan(bins)
        assert pool_plan(bins)[1] <= LDS_MAX


def test_the_limits(plan):
    """2,048 bins beside m = 4096 and K = 256: the keep pass takes one wave of 49 KiB, the rescore two of 24 KiB, the
    pool 16 KiB; one wave never exceeds 64 KiB for bins <= 2048 and m <= 4096."""
    assert plan(KEEP, 2048, 256, 4096) == (1, (2048 + 256 + 8192 + 2048) * 4, 0)
    assert plan(RESCORE, 2048, 0, 4096) == (2, 2 * 2048 * 12, 0)
    assert plan(RESCORE, 257, 0, 200) == (4, 4 * 257 * 12, 0)
    assert plan(POOL, 2048, 0, 4096) == (4, 2048 * 8, 0)
    for which in (KEEP, RESCORE, POOL):
        for bag_k in BAG_K:
            waves, lds, _ = plan(which, 2048, bag_k, 4096)
            assert lds // waves <= LDS_MAX if which != POOL else lds <= LDS_MAX
