"""Thinned pooling mapping v1 restated (tests/pool_draws_law.py) on hand-made kept samples, without a GPU: the contracts
K2, K3 and K4 hold in the restatement, the weights are thinned acceptance mapping v1's (tests/accept_draws_law.py), and
the cases the mapping names — a guard header, {0, 0}, a + b < m1, m1 = 1, m1 = a + b - 1 (a complement with one pick),
two targets of equal m1, an errored replicate, a held-out slot — each add what the text says."""
import numpy as np

import accept_draws_law as adl
import keep_law as kl
import pool_draws_law as pdl
import thin_law as tl

BINS, KEEP, SEED = 6, 12, 41
PER_SET, SETS = 5, 2
SIZES = (5, KEEP, 5, 1)  # two targets of equal m1, one scored whole on every replicate, one cell
KEPT = np.dtype([("nminus", np.uint32), ("nplus", np.uint32)])
SUMMARY = np.dtype([("error", np.uint32)])
FIRST, ND = 3, 6
INF = np.inf
GUARD_I, EMPTY_I, SMALL_I, FULL_I, ONE_PICK_I, ERR_I = 0, 1, 2, 3, 4, 5


def _samples():
    """Nine kept samples of at most 12 cells in two parameter sets (5 + 4)."""
    rng = np.random.default_rng(5)
    shapes = [(kl.GUARD, kl.GUARD),  # the guard
              (0, 0),                # an extinct replicate
              (1, 2),                # a + b = 3 < m1 = 5: scored whole by every slot but the one-cell one
              (4, 8),                # full
              (2, 4),                # a + b = 6 = m1 + 1 for the slots of 5 cells: a complement with one pick
              (3, 9),                # full, and the replicate has an error
              (0, 12), (7, 5), (5, 7)]
    headers = np.zeros(len(shapes), dtype=KEPT)
    cells = np.full((len(shapes), KEEP), 9, dtype=np.uint16)  # (cells past nplus are unspecified)
    for i, (a, b) in enumerate(shapes):
        headers[i] = (a, b)
        if b != kl.GUARD:
            row = np.sort(rng.integers(1, BINS + 3, b))  # some above the last bin
            if b:
                row[-1] = 300
            cells[i, :b] = row
    summ = np.zeros(len(shapes), dtype=SUMMARY)
    summ["error"][ERR_I] = 4
    return headers, cells, summ, np.arange(len(shapes), dtype=np.uint64)


def _targets():
    rng = np.random.default_rng(6)
    return rng.integers(1, 30, (len(SIZES), BINS)).astype(np.uint64)


def _slots(headers, cells, sizes=SIZES):
    t = _targets()
    return [adl.Slot(headers, cells, t[p], sizes[p], SEED) for p in range(len(sizes))]


def _thresholds(slots, ids, summ):
    """Row 0: a ks cut in a gap of the thinned records' distances, the gap under which most replicates pass some draws
    and fail others; row 1: everything off."""
    per_draw = [adl.records(slots, ids, BINS, d) for d in range(FIRST, FIRST + ND)]
    v = np.unique(np.concatenate([r["ks"].ravel() for r in per_draw]))
    best = None
    for cut in 0.5 * (v[1:] + v[:-1]):
        thr = [[float(cut), INF, INF, INF], [INF] * 4]
        ok = pdl.passing(slots, summ, ids, BINS, PER_SET, SETS, thr, 0, FIRST, ND, 0, per_draw).sum(axis=1)
        decided = int(((ok > 0) & (ok < ND)).sum())
        if best is None or decided > best[0]:
            best = (decided, thr)
    return best[1]


def _nk(headers):
    guard = (headers["nminus"] == kl.GUARD) & (headers["nplus"] == kl.GUARD)
    return np.where(guard, 0, headers["nminus"].astype(np.int64) + headers["nplus"])


def _pool(slots, headers, cells, summ, ids, thr, q, mask=0, **kw):
    return pdl.pool_draws(slots, [(headers, cells)], summ, ids, BINS, PER_SET, SETS, thr, q, FIRST, ND, mask, **kw)


def test_contracts_hold_in_the_restatement():
    headers, cells, summ, ids = _samples()
    slots = _slots(headers, cells)
    thr = _thresholds(slots, ids, summ)
    sets = (ids // np.uint64(PER_SET)).astype(np.int64)
    nk = _nk(headers)
    decided = 0
    for mask in (0, 0b0101, 0b1000):
        want_passes, _ = adl.accept_draws(slots, summ, ids, BINS, PER_SET, SETS, thr, FIRST, ND, mask)
        for q in (0, 1):
            thinned, kept, passes = _pool(slots, headers, cells, summ, ids, thr, q, mask)
            assert thinned.shape == (4, SETS, BINS) and kept.shape == (1, SETS, BINS)
            np.testing.assert_array_equal(passes, want_passes[:, q])  # the weights are accept_draws'
            np.testing.assert_array_equal(thinned[1], kept[0])  # K2: sample_cells == keep_cells
            np.testing.assert_array_equal(thinned[0], thinned[2])  # K4: equal m1 on one slice
            for slot, m1 in enumerate(SIZES):  # K3
                want = np.bincount(sets, weights=passes * np.minimum(m1, nk), minlength=SETS).astype(np.uint64)
                np.testing.assert_array_equal(thinned[slot].sum(axis=1), want)
            decided += int(((passes > 0) & (passes < ND)).sum())
            assert passes[ERR_I] == 0 and passes[GUARD_I] == ND  # (a guard's all-zero records pass every row)
    assert decided > 0  # some replicate passes some draws and not others


def test_each_named_case_adds_what_the_text_says():
    headers, cells, summ, ids = _samples()
    slots = _slots(headers, cells)
    thr = [[INF] * 4]

    def alone(i, **kw):
        """The pools of replicate i alone (every other replicate given an error), its set's rows."""
        s = summ.copy()
        s["error"] = 1
        s["error"][i] = summ["error"][i]
        thinned, kept, passes = _pool(slots, headers, cells, s, ids, thr, 0, **kw)
        assert not np.delete(passes, i).any()
        other = 1 - int(ids[i]) // PER_SET
        assert not thinned[:, other].any() and not kept[:, other].any()
        return thinned[:, int(ids[i]) // PER_SET], kept[0, int(ids[i]) // PER_SET], int(passes[i])

    # a guard header passes and adds nothing; an errored replicate passes nothing
    for i in (GUARD_I, ERR_I):
        thinned, kept, passes = alone(i)
        assert passes == (ND if i == GUARD_I else 0) and not thinned.any() and not kept.any()
    # {0, 0}: passes every draw of the all-off row and has no cell to add
    thinned, kept, passes = alone(EMPTY_I)
    assert passes == ND and not thinned.any() and not kept.any()
    # a + b = 3 < m1: the whole kept sample on every passing draw; the one-cell slot draws one of the three
    thinned, kept, passes = alone(SMALL_I)
    whole = kl.kept_hist((1, 2), cells[SMALL_I], BINS)
    np.testing.assert_array_equal(kept, np.uint64(ND) * whole)
    assert whole.sum() == 3 and whole[0] == 1 and whole[BINS - 1] >= 1  # (300 is clipped into the last bin)
    for slot in (0, 1, 2):
        np.testing.assert_array_equal(thinned[slot], np.uint64(ND) * whole)
    assert thinned[3].sum() == ND and np.all(thinned[3] <= np.uint64(ND) * whole)
    # m1 = a + b - 1: every draw leaves exactly one cell of the kept sample out
    thinned, kept, passes = alone(ONE_PICK_I)
    whole = kl.kept_hist((2, 4), cells[ONE_PICK_I], BINS)
    left_out = np.uint64(ND) * whole - thinned[0]
    assert left_out.sum() == ND and np.all(thinned[0] <= np.uint64(ND) * whole)
    hists = pdl.thinned_hists(slots[:1], ids, BINS, FIRST, ND)[0, ONE_PICK_I]
    assert np.all(hists.sum(axis=1) == 5) and len({h.tobytes() for h in hists}) > 1  # the draws differ
    # m1 = 1 on a full sample: one cell per passing draw
    thinned, kept, passes = alone(FULL_I)
    assert thinned[3].sum() == ND and thinned[0].sum() == 5 * ND and thinned[1].sum() == KEEP * ND
    # the draws of the range alone are pooled: another range gives other thinned samples, the same kept pool
    a = pdl.pool_draws(slots, [(headers, cells)], summ, ids, BINS, PER_SET, SETS, thr, 0, 0, ND)
    b = _pool(slots, headers, cells, summ, ids, thr, 0)
    assert (a[0][0] != b[0][0]).any() and np.array_equal(a[1], b[1]) and np.array_equal(a[0][1], b[0][1])


def test_a_held_out_slot_is_predicted_not_conditioned_on():
    headers, cells, summ, ids = _samples()
    slots = _slots(headers, cells)
    thr = _thresholds(slots, ids, summ)
    # slot 3 (one cell: the noisiest verdict) alone decides, or is held out
    with3, _, p_with = _pool(slots, headers, cells, summ, ids, thr, 0, 0b1000)
    without3, _, p_without = _pool(slots, headers, cells, summ, ids, thr, 0, 0b0111)
    assert with3[3].sum() == p_with[_nk(headers) > 0].sum() and without3[3].sum() == p_without[_nk(headers) > 0].sum()
    assert without3[3].sum() > 0 and (p_with != p_without).any()
    # held out, it is pooled on the draws the others pass: its histogram is that of its thinned samples on those draws
    ok = pdl.passing(slots, summ, ids, BINS, PER_SET, SETS, thr, 0, FIRST, ND, 0b0111)
    hists = pdl.thinned_hists(slots[3:], ids, BINS, FIRST, ND)[0]
    want = np.zeros((SETS, BINS), dtype=np.uint64)
    for i in range(len(ids)):
        want[int(ids[i]) // PER_SET] += hists[i, ok[i]].sum(axis=0, dtype=np.uint64)
    np.testing.assert_array_equal(without3[3], want)


def test_the_timepoint_store_pools_every_slice_under_its_own_stream():
    """Two slices of the same kept samples under different snapshot fields and keys: the thinned pools differ, the kept
    pools are per slice, and masking a slice out of the verdict leaves it in both pools."""
    headers, cells, summ, ids = _samples()
    t = _targets()
    slots = [adl.Slot(headers, cells, t[0], 5, SEED, snapshot=0), adl.Slot(headers[::-1], cells[::-1], t[1], 5, SEED,
                                                                            snapshot=1)]
    slices = [(headers, cells), (headers[::-1], cells[::-1])]
    s2 = np.zeros((len(ids), 2), dtype=SUMMARY)
    thr = [[INF] * 4]
    thinned, kept, passes = pdl.pool_draws(slots, slices, s2, ids, BINS, PER_SET, SETS, thr, 0, FIRST, ND, 0b01)
    assert np.all(passes == ND) and thinned.shape == kept.shape == (2, SETS, BINS)
    nk = _nk(headers)
    for j, order in enumerate((nk, nk[::-1])):
        sets = (ids // np.uint64(PER_SET)).astype(np.int64)
        np.testing.assert_array_equal(kept[j].sum(axis=1), np.bincount(sets, weights=ND * order, minlength=SETS))
        np.testing.assert_array_equal(thinned[j].sum(axis=1),
                                      np.bincount(sets, weights=ND * np.minimum(5, order), minlength=SETS))
    same_key = tl.thinned((4, 8), cells[FULL_I], 5, SEED, 3, 0, 0)
    other = tl.thinned((4, 8), cells[FULL_I], 5, SEED, 3, 0, 1)
    assert same_key[0] != other[0] or not np.array_equal(same_key[1], other[1])  # (the snapshot field moves the stream)
