"""The post-run passes' device buffers within one context (ecdna-evo_amd/csrc/ssa_ctx.hpp: DeviceBuf, TargetSet and the
per-pass states): reserved at a first call, outgrown by a larger one, reused by a smaller one.

One keep-block context and one timepoint-keep context (two snapshots) each run every post-run call three times, small,
large, small: accept, select, rescore, the sized rescore, pool_accepted, download_kept by ids, accept_draws, pool_draws
and select_draws. Every result is byte-equal to the same calls on a fresh context of the same spec, whose buffers were
first reserved at exactly that size (a context's seed is fixed at creation, so its records reproduce). Small: 1 target,
1 threshold row, 1 rank, 2 draws, 1 id, list capacity 0; large: 3 targets, 4 rows, 8 ranks, 8 draws, all ids, list
capacity n. (The timepoint store takes one target per timepoint, so its targets are two at either size.) The shapes are
those of tests/test_gpu_select_draws.py, on the row store."""
import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.draws_specs import KEEP, N, _spec, _targets
from support.gpu import _launched

INF = np.inf
BINS = 9
# (row 1, the large size's list row: every ks but the empty samples' 1.0)
ROWS = [[0.6, INF, INF, INF], [0.95, INF, INF, INF], [INF, 0.4, INF, 0.3], [INF] * 4]
FRACTIONS = (0.02, 0.1, 0.25, 0.4, 0.55, 0.7, 0.85, 1.0)
SIZES = {
    "small": dict(P=1, rows=ROWS[:1], list_row=0, fractions=FRACTIONS[3:4], draws=2, first=5, ids=[131], cap=0),
    "large": dict(P=3, rows=ROWS, list_row=1, fractions=FRACTIONS, draws=8, first=0, ids=list(range(N - 1, -1, -1)),
                  cap=N),
}
CELLS = (90, 130, 60)  # measured cells per target of the keep store (199 kept)
TP_CELLS = (20, 35)  # ... and per timepoint of the timepoint store (50 kept)


def _kept_bytes(headers, cells):
    """Headers and cell prefixes: the entries of a row past nplus are unspecified and set to zero here."""
    c = cells.copy()
    nplus = np.where(headers["nplus"] == abi.KEPT_GUARD, 0, headers["nplus"]).astype(np.int64)
    c[np.arange(c.shape[-1]) >= nplus[..., None]] = 0
    return headers.tobytes(), c.tobytes()


def _select_bytes(r):
    return r.population, r.ranks.tobytes(), r.values.tobytes(), r.counts_le.tobytes()


def _accept_bytes(a):
    return a.counts.tobytes(), a.mask.tobytes(), a.n_accepted, a.ids.tobytes(), a.stats.tobytes()


def _calls(ctx, store, size):
    """Every post-run call at one size, in an order that gives each what it needs; what each returned, by name."""
    z = SIZES[size]
    tp = store == "timepoints"
    P = 2 if tp else z["P"]
    t = _targets(BINS, 3)[:P]
    cells = TP_CELLS if tp else CELLS[:P]
    source = abi.ACCEPT_RESCORED_TIMEPOINTS if tp else abi.ACCEPT_RESCORED
    out = {}
    out["rescore"] = (ctx.rescore_timepoints(t) if tp else ctx.rescore(t)).tobytes()
    out["accept"] = _accept_bytes(ctx.accept(source, z["rows"], None, z["list_row"], z["cap"]))
    out["select"] = _select_bytes(ctx.select(source, fractions=z["fractions"]))
    out["pool_accepted"] = (ctx.pool_accepted_timepoints if tp else ctx.pool_accepted)(z["list_row"]).tobytes()
    out["download_kept"] = _kept_bytes(*(ctx.download_kept_timepoints if tp else ctx.download_kept)(ids=z["ids"]))
    out["rescore_sized"] = (ctx.rescore_timepoints(t, cells, 3) if tp else ctx.rescore(t, cells, [3] * P)).tobytes()
    out["select after the sized rescore"] = _select_bytes(ctx.select(source, fractions=z["fractions"]))
    adr = ctx.accept_draws(t, cells, z["rows"], z["draws"], z["first"], None, store)
    out["accept_draws"] = (adr.sums.tobytes(), adr.passes.tobytes())
    pool = ctx.pool_draws(t, cells, z["rows"], z["list_row"], z["draws"], z["first"], None, store)
    out["pool_draws"] = (pool.thinned.tobytes(), pool.kept.tobytes())
    out["select_draws"] = _select_bytes(ctx.select_draws(t, cells, z["draws"], z["first"], None, store,
                                                         fractions=z["fractions"]))
    # (the earlier results are still there: the later calls have buffers of their own)
    out["download_accept"] = _accept_bytes(ctx.download_accept())
    return out


SPECS = {
    "keep": dict(),
    "timepoints": dict(keep_cells=None, snapshots=(30, 160), snapshot_stats=True, keep_timepoint_cells=50),
}


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["keep", "timepoints"])
def test_buffers_are_reserved_outgrown_and_reused_within_one_context(engine_mod, store):
    spec = _spec("rows", 0, BINS, **SPECS[store])
    fresh = {}
    for size in SIZES:
        with _launched(engine_mod, spec) as ctx:
            fresh[size] = _calls(ctx, store, size)
    # the calls tell the sizes apart, and accept something
    assert len(fresh["large"]["accept_draws"][1]) == 4 * len(fresh["small"]["accept_draws"][1]) == 4 * N
    assert fresh["large"]["accept"][2] > 0 and fresh["large"]["select_draws"][0] > 100 * 8
    assert KEEP > max(CELLS) and SPECS["timepoints"]["keep_timepoint_cells"] > max(TP_CELLS)  # (the sizes thin)
    with _launched(engine_mod, spec) as ctx:
        for step, size in enumerate(("small", "large", "small")):
            got = _calls(ctx, store, size)
            for name, want in fresh[size].items():
                assert got[name] == want, f"{store} store, step {step} ({size}): {name}"
