"""The runs of the suites over thinning draws (tests/test_gpu_accept_draws.py, test_gpu_select_draws.py,
test_gpu_pool_draws.py, test_gpu_pass_buffers.py), which check one another on the same shapes, and the raw block of
ecdna_ssa_ctx_accept_draws."""
import ctypes as C

import numpy as np

from ecdna_evo_amd import abi
from support.gpu import _flags

INF = np.inf
TWO_STORES = [("rows", 0), ("bins", 64)]
SEED = 31
KEEP = 199
N, SETS, PER_SET = 258, 3, 86  # set and workgroup boundaries fall inside waves; 258 x 64 and 258 x 3 are no multiples of 256
RATES = ((1.0, 1.3, 0.4, 0.4), (1.0, 1.5, 0.4, 0.3), (1.1, 1.2, 0.5, 0.4))
SIZES = (90, 130, 90)  # picks over two batches, a complement, and a shared sample
FRACTIONS = (0.02, 0.1, 0.25, 0.4, 0.55, 0.7, 0.85, 1.0)


def _targets(bins, n=3):
    rng = np.random.default_rng(23)
    t = rng.integers(0, 70, (n, bins)).astype(np.uint64)
    t[:, 0] += 40
    t[:, bins - 1] = np.arange(n) % 4
    return t


def _spec(store, kmax, bins, **kw):
    """258 birth-death replicates in three parameter sets from three cells to 600 cells or time 6: some go extinct, some
    end small, most end above the kept sample's size."""
    base = dict(seed=SEED, process=abi.BIRTH_DEATH, rates=RATES, reps_per_set=PER_SET, n_replicates=N, max_cells=600,
                max_time=6.0, hist_bins=bins, init={0: 1, 1: 1, 12: 1}, flags=_flags(store), bin_kmax=kmax,
                keep_cells=KEEP)
    base.update(kw)
    return abi.RunSpec(**base)


def _nk(headers):
    return headers["nminus"].astype(np.int64) + headers["nplus"]


def _rows(values, Q=32):
    """Q threshold rows from select's values [4][K]: order statistics of the distances (so ties occur) mixed with +inf;
    the last row switches everything off, the one before takes the largest value of each distance."""
    assert np.all(np.isfinite(values))
    K = values.shape[1]
    rows = [[INF if (q + x) % 3 == 0 else float(values[x, (q * 3 + x) % K]) for x in range(4)] for q in range(Q)]
    if Q >= 2:
        rows[Q - 2] = [float(values[x, K - 1]) for x in range(4)]
    rows[Q - 1] = [INF] * 4
    return np.asarray(rows, dtype=np.float64)


def _gap_thresholds(values, picks):
    """Midpoints of gaps between adjacent distinct values, near the quantiles `picks`; every gap wider than 1e-9 of the
    larger of its upper end and 1 (the records' floats agree to 1e-12 relative)."""
    v = np.unique(values[np.isfinite(values)])
    out = []
    for f in picks:
        k = min(int(f * (len(v) - 1)), len(v) - 2)
        while k + 2 < len(v) and not (v[k + 1] - v[k] > 1e-9 * max(v[k + 1], 1.0)):
            k += 1
        assert v[k + 1] - v[k] > 1e-9 * max(v[k + 1], 1.0), (f, v[k], v[k + 1])
        out.append(0.5 * (v[k] + v[k + 1]))
    return out


def _block(hists, cells, thr, **kw):
    thr = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1, 4)
    cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.uint32)
    a = abi.AcceptDraws(struct_size=C.sizeof(abi.AcceptDraws), n_targets=hists.shape[0], n_draws=64,
                        n_thresholds=thr.shape[0])
    a.target_hists = hists.ctypes.data_as(C.POINTER(C.c_uint64))
    if cells is not None:
        a.sample_cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
    a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
    for k, v in kw.items():
        setattr(a, k, v)
    return a, (hists, cells, thr)
