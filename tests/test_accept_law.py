"""The numpy restatement of acceptance mapping v1 (tests/accept_law.py) on hand-made records: a tie passes, inf
switches a statistic off, a NaN distance fails unless the threshold is inf, an error replicate is rejected whatever the
thresholds, the timepoint mask is honoured, and the list is truncated while n_accepted keeps the whole count."""
import numpy as np
import pytest

import accept_law as al

INF = np.inf
REC = np.dtype([("mean", "<f8"), ("entropy", "<f8"), ("frequency", "<f8"), ("ks", "<f8"), ("mean_rel", "<f8"),
                ("entropy_rel", "<f8"), ("frequency_diff", "<f8"), ("cells", "<u8")])
SUMM = np.dtype([("error", "<u4")])


def _records(rows):
    """rows: [n][T][4] distances in the order of accept_law.FIELDS."""
    a = np.asarray(rows, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, None, :]
    out = np.zeros(a.shape[:2], dtype=REC)
    for k, f in enumerate(al.FIELDS):
        out[f] = a[:, :, k]
    return out


def _summ(errors):
    out = np.zeros(np.shape(errors), dtype=SUMM)
    out["error"] = errors
    return out


def _run(rows, thr, errors=None, **kw):
    rec = _records(rows)
    n = rec.shape[0]
    errors = np.zeros(n, dtype=np.uint32) if errors is None else errors
    kw.setdefault("reps_per_set", max(n, 1))
    kw.setdefault("ids", np.arange(n, dtype=np.uint64))
    kw.setdefault("n_sets", 1)
    return al.accept(rec, _summ(errors), thresholds=thr, **kw)


def test_a_tie_passes_and_the_next_double_above_fails():
    x = 0.3
    r = _run([[x, x, x, x], [np.nextafter(x, 1.0), x, x, x], [x, x, x, np.nextafter(x, 1.0)]], [[x, x, x, x]])
    assert r.mask.tolist() == [1, 0, 0] and r.counts.tolist() == [[1]]


def test_inf_switches_a_statistic_off():
    rows = [[0.9, 0.1, 0.1, 0.1], [0.1, 0.9, 0.1, 0.1], [0.1, 0.1, 0.9, 0.1], [0.1, 0.1, 0.1, 0.9]]
    thr = [[0.5] * 4] + [[INF if j == k else 0.5 for j in range(4)] for k in range(4)] + [[INF] * 4]
    r = _run(rows, thr)
    # row 0 rejects all; row 1 + k accepts exactly the replicate whose k-th distance is large; the all-inf row all
    assert r.mask.tolist() == [0b100010, 0b100100, 0b101000, 0b110000]
    assert r.counts[:, 0].tolist() == [0, 1, 1, 1, 1, 4]


def test_a_nan_distance_fails_unless_the_threshold_is_inf():
    nan = np.nan
    rows = [[nan, 0.0, 0.0, 0.0], [0.0, 0.0, nan, 0.0], [0.0, 0.0, 0.0, 0.0]]
    thr = [[1e300] * 4, [INF, 1.0, 1.0, 1.0], [1.0, 1.0, INF, 1.0], [INF] * 4]
    r = _run(rows, thr)
    assert r.mask.tolist() == [0b1010, 0b1100, 0b1111]


def test_an_error_replicate_is_rejected_under_all_inf_thresholds():
    r = _run([[0.0] * 4] * 4, [[INF] * 4], errors=np.asarray([0, 2, 0, 5], dtype=np.uint32), reps_per_set=2, n_sets=2)
    assert r.mask.tolist() == [1, 0, 1, 0] and r.counts.tolist() == [[1, 1]] and r.n_accepted == 2


def test_the_timepoint_mask_is_honoured():
    # [n][T = 3]: replicate 0 fails only at t = 1, replicate 1 only at t = 2, replicate 2 nowhere
    good, far = [0.1] * 4, [0.1, 0.1, 0.8, 0.1]
    rows = [[good, far, good], [good, good, far], [good, good, good]]
    thr = [[0.5] * 4]
    assert _run(rows, thr).mask.tolist() == [0, 0, 1]  # 0 = all T
    assert _run(rows, thr, timepoint_mask=0b111).mask.tolist() == [0, 0, 1]
    assert _run(rows, thr, timepoint_mask=0b101).mask.tolist() == [1, 0, 1]
    assert _run(rows, thr, timepoint_mask=0b011).mask.tolist() == [0, 1, 1]
    assert _run(rows, thr, timepoint_mask=0b001).mask.tolist() == [1, 1, 1]
    with pytest.raises(AssertionError):
        _run(rows, thr, timepoint_mask=0b1000)
    # one summary per timepoint (the passage sources): an error outside the participating phases does not count
    errs = np.asarray([[0, 0, 2], [0, 2, 0], [0, 0, 0]], dtype=np.uint32)
    assert _run([[good] * 3] * 3, thr, errors=errs).mask.tolist() == [0, 0, 1]
    assert _run([[good] * 3] * 3, thr, errors=errs, timepoint_mask=0b011).mask.tolist() == [1, 0, 1]


def test_the_list_is_truncated_and_n_accepted_is_whole():
    n = 10
    rows = [[0.1 if i % 3 else 0.9, 0.0, 0.0, 0.0] for i in range(n)]  # 0, 3, 6, 9 fail row 1
    ids = 5 + 3 * np.arange(n, dtype=np.uint64)
    kw = dict(ids=ids, reps_per_set=7, n_sets=5, list_threshold=1)
    thr = [[INF] * 4, [0.5, INF, INF, INF]]
    full = _run(rows, thr, list_capacity=n, **kw)
    assert full.n_accepted == 6 and full.index.tolist() == [1, 2, 4, 5, 7, 8]
    assert full.ids.tolist() == [8, 11, 17, 20, 26, 29]
    assert full.counts[1].tolist() == [0, 2, 2, 1, 1] and full.counts[0].tolist() == [1, 2, 3, 2, 2]
    cut = _run(rows, thr, list_capacity=4, **kw)
    assert cut.n_accepted == 6 and cut.index.tolist() == [1, 2, 4, 5] and cut.ids.tolist() == [8, 11, 17, 20]
    none = _run(rows, thr, list_capacity=0, **kw)
    assert none.n_accepted == 6 and none.index.size == 0 and none.ids.size == 0
    assert np.array_equal(none.mask, full.mask) and np.array_equal(cut.counts, full.counts)
