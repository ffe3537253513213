"""End-of-run subsampling (ABI v13, subsample mapping v1) without a GPU: the C ABI declares, exports
and validates it, and the numpy restatement the GPU tests compare against (tests/subsample_law.py) draws what the
mapping says and draws uniformly."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import subsample_law as sl
from ecdna_evo_amd import abi
from exact_law import chi2_lumped
from support.abi import declared, header_text, product_lib  # noqa: F401 (fixture)


def test_header_declares_and_library_exports_the_call(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_download_sample") == [
        "ecdna_ssa_ctx* c", "ecdna_rep_stats_t* out_stats", "uint64_t* out_sample_hist"]
    assert hasattr(product_lib, "ecdna_ssa_ctx_download_sample")
    assert "ecdna_ssa_ctx_download_sample" in engine.EXPORTS
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    names = [f for f, _ in abi.Params._fields_]
    assert names[-3:] == ["reserved0", "subsample_cells", "reserved1"]
    assert product_lib.ecdna_ssa_ctx_download_sample(None, None, None) == abi.E_INVALID


def _create(lib, p):
    h = C.c_void_p()
    rc = lib.ecdna_ssa_ctx_create(C.byref(p), C.byref(h))
    msg = lib.ecdna_ssa_last_error_message().decode()
    if rc == 0:
        lib.ecdna_ssa_ctx_destroy(h)
    return rc, msg


def test_create_rejects_bad_subsample_parameters(product_lib):
    """Before any device is touched: E_INVALID with a message, GPU or not."""
    s = abi.RunSpec(n_replicates=4, flags=0, subsample_cells=100)  # without FLAG_REP_STATS
    rc, msg = _create(product_lib, s.params())
    assert rc == abi.E_INVALID and "subsample_cells" in msg and "REP_STATS" in msg
    s = abi.RunSpec(n_replicates=4, flags=abi.FLAG_REP_STATS, subsample_cells=4097)
    rc, msg = _create(product_lib, s.params())
    assert rc == abi.E_INVALID and "subsample_cells" in msg and "4096" in msg
    s = abi.RunSpec(n_replicates=4, flags=abi.FLAG_REP_STATS, subsample_cells=100)
    p = s.params()
    p.reserved1 = 1
    rc, msg = _create(product_lib, p)
    assert rc == abi.E_INVALID and "reserved1" in msg
    # in range: whatever comes back (no device here, a context there), it is not a parameter error
    for m in (0, 1, 4096):
        rc, msg = _create(product_lib, abi.RunSpec(n_replicates=4, flags=abi.FLAG_REP_STATS, subsample_cells=m).params())
        assert rc in (abi.OK, abi.E_NODEVICE), (m, rc, msg)
    with pytest.raises(ValueError):
        abi.RunSpec(subsample_cells=1 << 32).params()
    with pytest.raises(ValueError):
        abi.RunSpec(subsample_cells=-1).params()


def test_create_refuses_initial_populations_of_2_to_32_cells(product_lib):
    """Populations are u32 (the bin stepper adds n- + n+ in 32 bits): an initial n- + n+ of 2^32 - 1 is accepted, its
    final state being the one that reaches the sampling passes' N >= 2^32 - 1 guard; 2^32 is refused with E_INVALID by
    ecdna_ssa_ctx_create and ecdna_ssa_run, shared or per set, and by RunSpec before the engine or the oracle runs."""
    small = dict(n_replicates=4, max_cells=10, cell_cap=64, flags=abi.FLAG_REP_STATS, subsample_cells=5)
    rc, msg = _create(product_lib, abi.RunSpec(init={0: 2**32 - 3, 1: 2}, **small).params())
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    rc, msg = _create(product_lib, abi.RunSpec(init_per_set=[{0: 2**32 - 1}], **small).params())
    assert rc in (abi.OK, abi.E_NODEVICE), (rc, msg)
    for nm, per_set in ((2**32 - 2, False), (2**32 - 2, True), (2**32, False), (2**40, True)):
        spec = abi.RunSpec(init={0: 5, 1: 2}, **small) if not per_set else \
            abi.RunSpec(init_per_set=[{0: 5, 1: 2}], **small)
        p = spec.params()  # (the spec itself refuses such a population: the field is set behind it)
        if per_set:
            nms = np.asarray([nm], dtype=np.uint64)
            p.init_set_nminus = nms.ctypes.data_as(C.POINTER(C.c_uint64))
        else:
            p.init_nminus = nm
        rc, msg = _create(product_lib, p)
        assert rc == abi.E_INVALID and "2^32" in msg and "initial cells" in msg, (nm, per_set, rc, msg)
        assert product_lib.ecdna_ssa_run(C.byref(p), None, None, None, None) == abi.E_INVALID
    for bad in (dict(init={0: 2**32 - 2, 1: 2}), dict(init={0: 2**32}), dict(init_per_set=[{0: 2**32 - 1, 7: 1}])):
        with pytest.raises(ValueError, match="2\\^32"):
            abi.RunSpec(**bad, **small).params()
    abi.RunSpec(init={0: 2**32 - 2, 1: 1}, **small).params()


def test_vector_philox_is_the_scalar_model():
    from support.host_law import _philox

    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2**32, (50, 4), dtype=np.uint64)
    ctr[0] = 0
    ctr[1] = 0xFFFFFFFF
    for seed in (0, 26, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0):
        got = sl.philox_blocks(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
        for i in range(len(ctr)):
            assert got[i].tolist() == _philox([int(x) for x in ctr[i]], [seed & 0xFFFFFFFF, seed >> 32])


def test_draws_follow_the_mapping_word_by_word():
    """Draw i: the four words of block (i, 0xC0000000 | t, rid) in order, Lemire's rejection, then block t + 1. N just
    above 2^31 rejects almost every second word, so later words and later blocks are reached."""
    from support.host_law import _philox

    seed, rid = 0x5EED0000ABCD, (7 << 32) | 9
    for N in (1, 2, 6, 40, 1000, 2**31 + 12345, 2**32 - 2):
        count = 200 if N == 2**31 + 12345 else 40
        got = sl.draws(5, count, N, seed, rid)
        later_word = later_block = 0
        for n, i in enumerate(range(5, 5 + count)):
            t, val = 0, None
            while val is None:
                for j, x in enumerate(_philox([i, 0xC0000000 | t, rid & 0xFFFFFFFF, rid >> 32],
                                              [seed & 0xFFFFFFFF, seed >> 32])):
                    p = x * N
                    if (p & 0xFFFFFFFF) >= (2**32 - N) % N:
                        val = p >> 32
                        later_word += j > 0
                        later_block += t > 0
                        break
                t += 1
            assert int(got[n]) == val and val < N
        if N == 2**31 + 12345:
            assert later_word and later_block


@pytest.mark.parametrize("N,m", [(6, 3), (6, 4)])
def test_restatement_samples_uniformly(N, m):
    """Every m-subset of the N positions equally often over 20,000 replicate ids (m = 4 through the complement)."""
    subsets = {s: 0 for s in itertools.combinations(range(N), m)}
    for rid in range(20000):
        pos, comp = sl.sample_positions(N, m, 77, rid)
        assert comp == (m > N - m)
        assert len(pos) == min(m, N - m) == len(set(pos.tolist())) and pos.min() >= 0 and pos.max() < N
        kept = sorted(set(range(N)) - set(pos.tolist())) if comp else sorted(pos.tolist())
        subsets[tuple(kept)] += 1
    obs = np.asarray(list(subsets.values()))
    assert len(obs) == (20 if m == 3 else 15)
    p = chi2_lumped(obs, np.full(len(obs), 20000 / len(obs)), min_expected=5)
    assert p > 1e-6, (p, obs)


def test_restatement_edges():
    for N, m in ((0, 5), (1, 1), (5, 5), (5, 9), (40, 4096)):  # m >= N: everything, in order
        pos, comp = sl.sample_positions(N, m, 1, 2)
        assert pos.tolist() == list(range(N)) and not comp
    for N, m in ((2, 1), (41, 20), (41, 21), (2000, 1999), (2000, 1), (8200, 4096), (65, 64)):
        for rid in (0, 1, 2**40 + 3):
            pos, comp = sl.sample_positions(N, m, 9, rid)
            assert len(pos) == min(m, N - m) == len(np.unique(pos)) and pos.max() < N and comp == (m > N - m)
    # a sample depends on (N, m, seed, rid) only, and changes with each of them
    a = sl.sample_positions(1000, 100, 5, 6)[0]
    assert np.array_equal(a, sl.sample_positions(1000, 100, 5, 6)[0])
    for other in ((1001, 100, 5, 6), (1000, 100, 4, 6), (1000, 100, 5, 7)):
        assert not np.array_equal(a, sl.sample_positions(*other)[0])
    assert np.array_equal(a[:50], sl.sample_positions(1000, 50, 5, 6)[0])  # the same draw sequence, cut earlier


def test_sample_statistics_are_those_of_the_sampled_cells():
    import abc_stats

    rng = np.random.default_rng(11)
    row = rng.integers(1, 400, 150)
    nminus, bins = 50, 257
    tgt = np.zeros(bins, np.uint64)
    tgt[:30] = 7
    full = abc_stats.rep_stats(nminus, row, bins, tgt)
    assert sl.sample_stats(nminus, row, 200, 3, 4, bins, tgt) == full  # m = N
    assert sl.sample_stats(nminus, row, 4096, 3, 4, bins, tgt) == full
    assert np.array_equal(sl.sample_hist(nminus, row, 200, 3, 4, bins),
                          np.bincount(np.minimum(row, bins - 1), minlength=bins) + np.eye(1, bins, 0, dtype=int)[0] * 50)
    for m in (1, 60, 100, 140, 199):  # 140 and 199 through the complement
        nm_s, row_s = sl.sample_cells(nminus, row, m, 3, 4)
        assert nm_s + len(row_s) == m
        st = sl.sample_stats(nminus, row, m, 3, 4, bins, tgt)
        assert st["cells"] == m and st == abc_stats.rep_stats(nm_s, row_s, bins, tgt)
        assert int(sl.sample_hist(nminus, row, m, 3, 4, bins).sum()) == m
        # the sample is a sub-multiset of the population
        cnt = np.bincount(row, minlength=400) - np.bincount(row_s, minlength=400)
        assert cnt.min() >= 0 and nm_s <= nminus
    assert sl.sample_stats(0, [], 10, 3, 4, bins, tgt)["ks"] == 1.0  # extinct: as the full statistics


@pytest.mark.parametrize("shape", ["rows", "counters", "both"])
def test_described_states_sample_as_their_expansion(shape):
    """The position -> copy number map of a described state (N- cells, counters k = 1..K ascending, row; searchsorted
    on the prefix sums, nothing expanded) against sample_cells on the same state written out cell by cell: rows only,
    counters only (with empty counters between full ones) and both, at N around m, 2m - 1 and 2m (the whole population,
    the complement down to m' = 1 and up to m' = m - 1, the first direct sample), with and without N- cells."""
    rng = np.random.default_rng(23)
    m, bins = 64, 33
    tgt = np.zeros(bins, np.uint64)
    tgt[:20] = 5
    for N in (m - 1, m, m + 1, 2 * m - 2, 2 * m - 1, 2 * m, 2 * m + 1, 5 * m):
        for nminus in (0, 7):
            nplus = N - nminus
            n_row = {"rows": nplus, "counters": 0, "both": nplus // 3}[shape]
            row = rng.integers(33, 400, n_row)
            K = 0 if shape == "rows" else 32
            counters = np.zeros(K, np.int64)
            if K:  # nplus - n_row cells over a third of the counters: most counters stay empty
                np.add.at(counters, rng.choice(K, 10, replace=False)[rng.integers(0, 10, nplus - n_row)], 1)
            expanded = np.concatenate([np.repeat(np.arange(1, K + 1), counters), row]).astype(np.int64)
            assert len(expanded) == nplus
            pos = np.arange(N)
            k_all = sl.described_k(nminus, counters, row, pos)
            assert np.array_equal(k_all, np.concatenate([np.zeros(nminus, np.int64), expanded]))
            assert sl.described_k(nminus, counters, row, [N, N + 5]).tolist() == [-1, -1]
            for rid in (0, 2**40 + 5):
                want = sl.sample_cells(nminus, expanded, m, 2027, rid)
                got = sl.described_sample_cells(nminus, counters, row, m, 2027, rid)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), (N, nminus, rid)
                assert got[0] + len(got[1]) == min(m, N)
                assert sl.described_sample_stats(nminus, counters, row, m, 2027, rid, bins, tgt) == \
                    sl.sample_stats(nminus, expanded, m, 2027, rid, bins, tgt)
                assert np.array_equal(sl.described_sample_hist(nminus, counters, row, m, 2027, rid, bins),
                                      sl.sample_hist(nminus, expanded, m, 2027, rid, bins))


def test_described_states_guards_and_trace():
    """The guards of a described state, and the draw trace's bookkeeping against the draws themselves."""
    zero = sl.described_sample_stats(0, [], [], 5, 1, 2, 17)
    assert zero["cells"] == 0
    row = np.arange(1, 301)
    assert sl.described_sample_cells(10, [], row, 100, 1, 2) is not None
    assert sl.described_sample_cells(2**32 - 1 - 300, [], row, 100, 1, 2) is None  # N = 2^32 - 1
    assert sl.described_sample_cells(2**33, [], row, 100, 1, 2) is None
    assert sl.described_sample_cells(2**32 - 2 - 300, [], row, 100, 1, 2) is not None  # N = 2^32 - 2: sampled
    assert sl.described_sample_cells(10, [200, 200], [], 100, 1, 2, nplus=399) is None  # counters above the summary
    assert sl.described_sample_cells(0, [], row[:64], 100, 1, 2, nplus=300) is None  # a summary beyond the row
    assert sl.described_sample_cells(10, [], row, 100, 1, 2, table_slots=128) is None  # m' = 100 needs 256 slots
    assert sl.described_sample_cells(10, [], row, 100, 1, 2, table_slots=256) is not None
    assert sl.described_sample_stats(10, [], row, 100, 1, 2, 17, table_slots=128) == zero
    assert not sl.described_sample_hist(10, [], row, 100, 1, 2, 17, table_slots=128).any()
    for N in (1000, 3 * 2**30, 2**31 + 12345):
        val, blocks, rejected = sl.draw_trace(3, 500, N, 77, 2**40 + 5)
        assert np.array_equal(val, sl.draws(3, 500, N, 77, 2**40 + 5)) and val.max() < N
        assert np.array_equal(blocks, rejected // 4 + 1) and blocks.min() == 1
        assert (rejected > 0).any() == (N > 1000)
