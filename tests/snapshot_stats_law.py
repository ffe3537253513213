"""TEST INFRASTRUCTURE ONLY — numpy restatement of the per-snapshot ABC statistics (ecdna_ssa_ext_t, include/ecdna_ssa.h;
DESIGN.md §3.4), written from the text of the header and not from the kernel.

The state saved at snapshot s is the snapshot's n- N- cells followed by its N+ row; a snapshot that was not taken is an
empty population. Its statistics are oracle/abc_stats.py's against snapshot s's own target. Its sample of m cells is
subsample mapping v1 (tests/subsample_law.py) over that population with one difference, the stream: draw i of
snapshot s reads Philox counter (i, 0xC0000000 | (s + 1) << 16 | t, rid lo, rid hi). The draw and the first-m'-distinct
rule are restated here because they carry the tag; Philox itself is subsample_law.philox_blocks.
"""
from functools import lru_cache

import numpy as np

import abc_stats
import subsample_law as sl

_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def stream_field(s):
    """The stream field of counter word 1 for snapshot s (the end-of-run sample's is 0)."""
    assert 0 <= s < 64
    return (s + 1) << 16


def draws(first, count, N, seed, rid, field):
    """Draws u_first .. u_(first + count - 1) below N on the stream `field`."""
    idx = np.arange(first, first + count, dtype=np.uint64)
    out = np.zeros(count, dtype=np.uint64)
    todo = np.arange(count)
    thr = np.uint64((2**32 - N) % N)
    t = 0
    while len(todo):
        assert t < 1024
        w = sl.philox_blocks(idx[todo], sl.TAG | field | t, rid & 0xFFFFFFFF, (rid >> 32) & 0xFFFFFFFF, seed)
        p = w * np.uint64(N)
        ok = (p & _MASK) >= thr
        got = ok.any(axis=1)
        first_ok = ok.argmax(axis=1)
        out[todo[got]] = p[got, first_ok[got]] >> _S32
        todo = todo[~got]
        t += 1
    return out


@lru_cache(maxsize=None)
def _picked(N, mp, seed, rid, field):
    """The first mp distinct values of the stream's draw sequence, in draw order (None under the 2^16-draw guard)."""
    seq = np.zeros(0, dtype=np.uint64)
    while True:
        _, first = np.unique(seq, return_index=True)
        if len(first) >= mp:
            return tuple(int(x) for x in seq[np.sort(first)[:mp]])
        if len(seq) >= sl.MAX_DRAWS:
            return None
        more = min(sl.MAX_DRAWS - len(seq), max(64, 2 * mp))
        seq = np.concatenate([seq, draws(len(seq), more, N, seed, rid, field)])


def sample_positions(N, m, seed, rid, s, field=None):
    """(positions, complement) of the sample of snapshot s, as subsample_law.sample_positions; `field` overrides the
    stream field of s (tests)."""
    N, m = int(N), int(m)
    if m >= N:
        return np.arange(N, dtype=np.int64), False
    mp = min(m, N - m)
    pk = _picked(N, mp, int(seed), int(rid), stream_field(s) if field is None else int(field))
    if pk is None:
        return None, False
    return np.asarray(pk, dtype=np.int64), mp != m


def state(meta, row):
    """(n-, N+ copy numbers) of a snapshot: its record (abi.SNAPSHOT_DTYPE) and its row; not taken: nothing."""
    if not int(meta["taken"]):
        return 0, np.zeros(0, dtype=np.int64)
    return int(meta["nminus"]), np.asarray(row, dtype=np.int64)[: int(meta["nplus"])]


def sample_cells(nminus, row, m, seed, rid, s):
    """(n-, N+ copy numbers) of the sample of m cells of the population (nminus N- cells, then row), or None."""
    nminus = int(nminus)
    row = np.asarray(row, dtype=np.int64)
    N = nminus + len(row)
    pos, comp = sample_positions(N, m, seed, rid, s)
    if pos is None:
        return None
    if comp:
        keep = np.ones(N, dtype=bool)
        keep[pos] = False
        pos = np.flatnonzero(keep)
    return int((pos < nminus).sum()), row[pos[pos >= nminus] - nminus]


def hist_of(nminus, row, bins):
    h = np.bincount(np.minimum(np.asarray(row, dtype=np.int64), bins - 1), minlength=bins).astype(np.uint64)
    h[0] += np.uint64(nminus)
    return h


def full(meta, row, bins, target=None):
    """(statistics, histogram) of the state saved at a snapshot."""
    nm, cells = state(meta, row)
    return abc_stats.rep_stats(nm, cells, bins, target), hist_of(nm, cells, bins)


def sample(meta, row, m, seed, rid, s, bins, target=None):
    """(statistics, histogram) of the sample of m cells of the state saved at snapshot s (all zero under the guard)."""
    nm, cells = state(meta, row)
    sc = sample_cells(nm, cells, m, seed, rid, s)
    if sc is None:
        return dict(cells=0, mean=0.0, entropy=0.0, frequency=0.0, ks=0.0, mean_rel=0.0, entropy_rel=0.0,
                    frequency_diff=0.0), np.zeros(bins, dtype=np.uint64)
    return abc_stats.rep_stats(sc[0], sc[1], bins, target), hist_of(sc[0], sc[1], bins)
