"""The accepted thinnings pooled (ecdna_ssa_ctx_pool_draws, added within ABI v13; thinned pooling mapping v1, DESIGN.md
§3.4) without a GPU: the header declares the call, the library exports it, the ctypes prototype is the header's, the
version is still 13, the header states the mapping, a bad call is ECDNA_E_INVALID with the field named before a device
is touched, and engine.Context.pool_draws checks its arguments."""
import ctypes as C
import re

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.abi import HEADER, declared, header_text, layout, product_lib  # noqa: F401 (fixture)
from support.draws_specs import _block

BINS = 9
INF = np.inf


def test_header_declares_and_library_exports_the_call(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_pool_draws") == [
        "ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a", "uint32_t threshold", "uint64_t* out_thinned",
        "uint64_t* out_kept"]
    # the calls it stands beside did not change
    assert declared("ecdna_ssa_ctx_accept_draws") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_draws_t* a"]
    assert declared("ecdna_ssa_ctx_pool_accepted") == ["ecdna_ssa_ctx* c", "uint32_t threshold",
                                                              "uint64_t* out_hist"]
    assert hasattr(product_lib, "ecdna_ssa_ctx_pool_draws") and "ecdna_ssa_ctx_pool_draws" in engine.EXPORTS
    want = [C.c_void_p, C.POINTER(abi.AcceptDraws), C.c_uint32, C.c_void_p, C.c_void_p]
    assert abi.POOL_DRAWS_ARGTYPES == want
    assert product_lib.ecdna_ssa_ctx_pool_draws.argtypes == want
    assert product_lib.ecdna_ssa_ctx_pool_draws.restype == C.c_int
    # additive: the version is v13's and the block kept its size
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13 and C.sizeof(abi.AcceptDraws) == 72


def test_null_arguments_are_invalid_as_accept_draws_says(product_lib):
    """Without a context (and so without a GPU) the call answers what ecdna_ssa_ctx_accept_draws answers."""
    L = product_lib
    hists = np.ones((1, BINS), dtype=np.uint64)
    out = np.zeros((1, 1, BINS), dtype=np.uint64)
    blk, alive = _block(hists, (5,), [[INF] * 4])
    sibling = L.ecdna_ssa_ctx_accept_draws(None, C.byref(blk))
    rc = L.ecdna_ssa_ctx_pool_draws(None, C.byref(blk), 0, out.ctypes.data, out.ctypes.data)
    assert rc == sibling == abi.E_INVALID
    assert L.ecdna_ssa_last_error_message()
    assert L.ecdna_ssa_ctx_pool_draws(None, None, 0, None, None) == abi.E_INVALID


def test_a_bad_call_names_its_field_before_a_device_is_touched(product_lib):
    """A keep context where there is a device, ECDNA_E_NODEVICE where there is none — and then the call on it, before
    any launch: a bad block, row or pair of outputs is ECDNA_E_INVALID with the field named, a good call
    ECDNA_E_STATE."""
    L = product_lib
    m = 20
    spec = abi.RunSpec(n_replicates=4, max_cells=50, hist_bins=BINS, flags=abi.FLAG_REP_STATS, keep_cells=m)
    p, k, h = spec.params(), spec.keep(), C.c_void_p()
    rc = L.ecdna_ssa_ctx_create_keep(C.byref(p), None, None, None, C.byref(k), C.byref(h))
    assert rc in (abi.OK, abi.E_NODEVICE)
    if rc != abi.OK:
        return
    try:
        two = np.ones((2, BINS), dtype=np.uint64)
        out = np.zeros((2, 1, BINS), dtype=np.uint64)
        ok_thr = [[0.5, INF, 0.0, 1.0], [INF] * 4]

        def call(q, thinned, kept, *a, **kw):
            blk, alive = _block(*a, **kw)
            rc = L.ecdna_ssa_ctx_pool_draws(h, C.byref(blk), q, thinned, kept)
            return rc, L.ecdna_ssa_last_error_message().decode()

        def refused(word, *a, q=0, thinned=out.ctypes.data, kept=out.ctypes.data, **kw):
            rc, msg = call(q, thinned, kept, *a, **kw)
            assert rc == abi.E_INVALID and word in msg, (word, rc, msg)

        assert L.ecdna_ssa_ctx_pool_draws(h, None, 0, out.ctypes.data, None) == abi.E_INVALID
        assert b"pool_draws: the block is NULL" in L.ecdna_ssa_last_error_message()
        # everything accept_draws refuses, with its messages
        refused("accept_draws.struct_size", two, (5, 5), ok_thr, struct_size=C.sizeof(abi.AcceptDraws) + 8)
        refused("accept_draws.reserved", two, (5, 5), ok_thr, reserved=1)
        refused("accept_draws.timepoints", two, (5, 5), ok_thr, timepoints=2)
        refused("accept_draws.n_targets", two, (5, 5), ok_thr, n_targets=0)
        holed = two.copy()
        holed[1] = 0
        refused("accept_draws.target_hists[1]", holed, (5, 5), ok_thr)
        refused("accept_draws.sample_cells is NULL", two, None, ok_thr)
        refused("accept_draws.sample_cells[1]", two, (5, m + 1), ok_thr)
        refused("accept_draws.n_draws", two, (5, 5), ok_thr, n_draws=65)
        refused("accept_draws.first_draw", two, (5, 5), ok_thr, first_draw=1)
        refused("accept_draws.n_thresholds", two, (5, 5), ok_thr, n_thresholds=0)
        refused("accept_draws.thresholds[0].ks", two, (5, 5), [[np.nan, 0, 0, 0]])
        refused("accept_draws.timepoint_mask", two, (5, 5), ok_thr, timepoint_mask=0b100)
        # the call's own arguments
        refused("pool_draws.threshold must be < accept_draws.n_thresholds = 2", two, (5, 5), ok_thr, q=2)
        refused("pool_draws.threshold", two, (5, 5), ok_thr, q=0xFFFFFFFF)
        refused("pool_draws.out_thinned and pool_draws.out_kept are both NULL", two, (5, 5), ok_thr, thinned=None,
                kept=None)
        # a good call, with either output alone: the state decides
        for thinned, kept in ((out.ctypes.data, out.ctypes.data), (out.ctypes.data, None), (None, out.ctypes.data)):
            rc, msg = call(1, thinned, kept, two, (5, m), ok_thr)
            assert rc == abi.E_STATE and "pool_draws before launch" in msg
        rc, msg = call(0, out.ctypes.data, None, two, (5, m), ok_thr, timepoints=1)
        assert rc == abi.E_STATE and "create_keep_timepoints" in msg
    finally:
        L.ecdna_ssa_ctx_destroy(h)


class _NoDevice:
    """What Context.pool_draws reads of a context before it calls the library."""

    def __init__(self, engine, bins):
        self.params = abi.RunSpec(n_replicates=4, max_cells=50, hist_bins=bins, flags=abi.FLAG_REP_STATS,
                                  keep_cells=20).params()
        self.h = None
        self._u32_list = engine.Context._u32_list
        self._accept_draws_block = lambda *a: engine.Context._accept_draws_block(self, *a)


def test_engine_argument_checks(product_lib):
    """Context.pool_draws refuses what it can see is wrong before the library is asked, as accept_draws does."""
    from ecdna_evo_amd import engine

    ctx = _NoDevice(engine, BINS)
    two = np.ones((2, BINS), dtype=np.uint64)
    thr = [[0.5, INF, 0.0, 1.0], [INF] * 4]
    pool = lambda *a, **kw: engine.Context.pool_draws(ctx, *a, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="store"):
        pool(two, (5, 5), thr, store="snapshots")
    with pytest.raises(ValueError, match="targets must be"):
        pool(np.ones((2, BINS + 1), dtype=np.uint64), (5, 5), thr)
    with pytest.raises(ValueError, match="thresholds must be"):
        pool(two, (5, 5), [0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="sample_cells"):
        pool(two, (5, 5, 5), thr)
    with pytest.raises(ValueError, match="n_draws"):
        pool(two, (5, 5), thr, n_draws=-1)
    with pytest.raises(ValueError, match="threshold = 2"):
        pool(two, (5, 5), thr, threshold=2)
    with pytest.raises(ValueError, match="threshold"):
        pool(two, (5, 5), thr, threshold=-1)
    # what is left the library refuses: without a context, ECDNA_E_INVALID
    with pytest.raises(engine.EngineError, match="ctx is NULL"):
        pool(two, (5, 5), thr, threshold=1)
    assert engine.PoolDrawsResult(1, 2).thinned == 1 and engine.PoolDrawsResult(1, 2).kept == 2


def test_the_header_states_thinned_pooling_mapping_v1():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Thinned pooling mapping v1",
                   "The block means what it means for ecdna_ssa_ctx_accept_draws",
                   "threshold is a row q < Q",
                   "Replicate i passes row q on draw d exactly when thinned acceptance mapping v1 says so",
                   "Nothing of that mapping or of thinning mapping v1 changes",
                   "a held-out biopsy or timepoint is predicted, not conditioned on",
                   "the sample thinning mapping v1 defines for (sample_cells[slot], d) on the slot's slice",
                   "when m1 >= a + b it is the whole kept sample, on every passing draw",
                   "bin 0 holds the N- cells, true copy numbers are clipped at hist_bins - 1",
                   "A guard header, a size the plan refuses and the 2^16-draw guard add nothing",
                   "n_slices is 1 on the keep store and T on the timepoint store",
                   "passes[i][q] times the histogram of i's whole kept sample of the slice",
                   "K1.", "K2.", "K3.", "K4.", "K5. Shards' arrays sum to the whole run's",
                   "It needs neither an earlier ecdna_ssa_ctx_accept_draws nor a rescore",
                   "A relaunch invalidates nothing of this call: it holds no result",
                   "threshold >= n_thresholds; both outputs NULL"):
        assert phrase in text, phrase
    assert "Added within v13 (additive: no layout and no existing function changes, the version stays 13): the " \
           "accepted thinnings pooled" in text
