"""What several suites of GPU tests share, whatever their shapes: the flags of a scored run, a launched context, the
comparisons of two results, the thresholds taken from a run's own distances. Each function stands here as the suites
had it; the runs that two or more suites share are in the *_specs modules beside this one, one per suite of origin."""
import ctypes as C
import dataclasses
import socket

import numpy as np

import accept_law as al
import keep_law as kl
from cases import cases
from ecdna_evo_amd import abi

INF = np.inf
FRACS = (0.10, 0.25, 0.50, 0.75, 0.90)
ALL_INF_ROW = len(FRACS)  # the row after the order statistics
R = abi.FLAG_REFERENCE_DRAWS


def _flags(store):
    return abi.FLAG_REP_STATS | abi.FLAG_EVENT_HASH | (abi.FLAG_BIN_STORE if store == "bins" else 0)


def _thresholds(records, summaries, fracs=FRACS):
    """The order statistics of each distance among the error-free replicates, the all-inf row, the ks = 0 row."""
    err = summaries["error"]
    ok = err == 0 if err.ndim == 1 else (err == 0).all(axis=1)
    rec = records[ok]
    assert rec.size, "no error-free replicate"
    rows = []
    for f in fracs:
        row = []
        for name in al.FIELDS:
            v = np.sort(rec[name].ravel())
            row.append(float(v[int(f * (len(v) - 1))]))
        rows.append(row)
    return np.asarray(rows + [[INF] * 4, [0.0, INF, INF, INF]], dtype=np.float64)


def _run(engine_mod, spec):
    ctx = engine_mod.Context(spec)
    ctx.launch()
    ctx.sync()
    return ctx, ctx.download()


def _launched(engine_mod, spec):
    ctx = engine_mod.Context(spec)
    ctx.launch()
    ctx.sync()
    return ctx


def _same_accept(got, want, tag):
    np.testing.assert_array_equal(got.counts, want.counts, err_msg=tag)
    np.testing.assert_array_equal(got.mask, want.mask, err_msg=tag)
    assert got.n_accepted == want.n_accepted, tag
    np.testing.assert_array_equal(got.ids, want.ids, err_msg=tag)


def _same_select(got, want, tag):
    assert got.population == want.population, tag
    np.testing.assert_array_equal(got.ranks, want.ranks, err_msg=tag)
    np.testing.assert_array_equal(got.values.view(np.uint64), want.values.view(np.uint64), err_msg=tag)
    np.testing.assert_array_equal(got.counts_le, want.counts_le, err_msg=tag)


def _canon(headers, cells):
    """Headers and cell prefixes as bytes: entries past nplus are unspecified and set to zero here."""
    c = cells.copy()
    guard = headers["nplus"] == kl.GUARD
    nplus = np.where(guard, 0, headers["nplus"]).astype(np.int64)
    c[np.arange(c.shape[1])[None, :] >= nplus[:, None]] = 0
    return headers.tobytes() + c.tobytes()


def _source_codes(L, h, source):
    thr = np.asarray([[INF] * 4])
    a = abi.Accept(struct_size=C.sizeof(abi.Accept), source=source, n_thresholds=1)
    a.thresholds = thr.ctypes.data_as(C.POINTER(abi.AcceptThreshold))
    rk = (C.c_uint64 * 1)(1)
    s = abi.Select(struct_size=C.sizeof(abi.Select), source=source, n_ranks=1)
    s.ranks = C.cast(rk, C.POINTER(C.c_uint64))
    pre, hist = np.zeros((4, 1), dtype=np.uint64), np.zeros((4, 1, 256), dtype=np.uint64)
    return (L.ecdna_ssa_ctx_accept(h, C.byref(a)), L.ecdna_ssa_ctx_select(h, C.byref(s), None, None, None, None),
            L.ecdna_ssa_ctx_select_digits(h, source, 0, 0, 1, pre.ctypes.data, hist.ctypes.data))


def _compare(gpu, cpu, name):
    gs, cs = gpu.summaries, cpu.summaries
    for f in gs.dtype.names:
        if f == "time":
            np.testing.assert_array_equal(gs[f].view(np.uint64), cs[f].view(np.uint64), err_msg=f"{name}: {f}")
        else:
            np.testing.assert_array_equal(gs[f], cs[f], err_msg=f"{name}: {f}")
    for i in range(len(gs)):
        np.testing.assert_array_equal(gpu.row(i), cpu.row(i), err_msg=f"{name}: row {i}")
    np.testing.assert_array_equal(gpu.hist, cpu.hist, err_msg=f"{name}: hist")
    for f in gpu.totals.dtype.names:
        np.testing.assert_array_equal(gpu.totals[f], cpu.totals[f], err_msg=f"{name}: totals.{f}")
    if cpu.snapshots is not None:
        for f in ("nminus", "nplus", "taken"):
            np.testing.assert_array_equal(gpu.snapshots[f], cpu.snapshots[f], err_msg=f"{name}: snapshots.{f}")
        np.testing.assert_array_equal(gpu.snapshots["time"].view(np.uint64), cpu.snapshots["time"].view(np.uint64))
        if cpu.snapshot_rows is not None:
            for i in range(len(gs)):
                for s in range(cpu.snapshots.shape[1]):
                    np.testing.assert_array_equal(gpu.snapshot_row(i, s), cpu.snapshot_row(i, s),
                                                  err_msg=f"{name}: snapshot row {i}/{s}")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bytes_of(r):
    return (r.population, r.ranks.tobytes(), r.values.tobytes(), r.counts_le.tobytes())


def refdraws_cases():
    return {name: dataclasses.replace(spec, flags=spec.flags | R, _keep=[]) for name, spec in cases().items()}
