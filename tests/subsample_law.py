"""TEST INFRASTRUCTURE ONLY — numpy restatement of the engine's end-of-run subsample (subsample mapping v1,
include/ecdna_ssa.h), written from the text of the mapping and not from the kernel.

A replicate's final population of N = n- + n+ cells is numbered 0..N-1 in download order (the N- cells, then the
row as ecdna_ssa_ctx_download returns it). For m < N, m' = min(m, N - m) positions are picked: the first m' distinct
values of the draw sequence u_0, u_1, ..., each a Lemire draw below N from Philox4x32-10 under the run's key on counter
(i, 0xC0000000 | t, rid lo, rid hi). They are the sample when m' = m and the cells left out otherwise. Philox is
vectorised over the draw index (the scalar model is `_philox` in tests/test_host.py). The statistics are
oracle/abc_stats.py's, applied to the sampled cells.
"""
from functools import lru_cache

import numpy as np

import abc_stats

MAX_DRAWS = 1 << 16  # the guard: a replicate that has not finished after this many draws gets all-zero statistics
TAG = 0xC0000000
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_blocks(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) (arrays or scalars) under key (seed lo, seed hi): [n][4] u64."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in (c0, c1, c2, c3)]
    n = max(len(x) for x in c)
    c = [np.broadcast_to(x, (n,)).copy() for x in c]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [((p1 >> _S32) ^ c[1] ^ np.uint64(k0)) & _MASK, p1 & _MASK, ((p0 >> _S32) ^ c[3] ^ np.uint64(k1)) & _MASK,
             p0 & _MASK]
    return np.stack(c, axis=1)


def draw_trace(first, count, N, seed, rid):
    """Draws u_first .. u_(first + count - 1) below N, the Philox blocks each took (1 = none wholly rejected) and how
    many words each rejected before its accepted one."""
    idx = np.arange(first, first + count, dtype=np.uint64)
    out = np.zeros(count, dtype=np.uint64)
    blocks = np.zeros(count, dtype=np.int64)
    rejected = np.zeros(count, dtype=np.int64)
    todo = np.arange(count)
    thr = np.uint64((2**32 - N) % N)
    t = 0
    while len(todo):
        w = philox_blocks(idx[todo], TAG | t, rid & 0xFFFFFFFF, (rid >> 32) & 0xFFFFFFFF, seed)
        p = w * np.uint64(N)  # x * N < 2^64
        ok = (p & _MASK) >= thr
        got = ok.any(axis=1)
        first_ok = ok.argmax(axis=1)
        out[todo[got]] = (p[got, first_ok[got]] >> _S32)
        blocks[todo] = t + 1
        rejected[todo] += np.where(got, first_ok, 4)
        todo = todo[~got]
        t += 1
    return out, blocks, rejected


def draws(first, count, N, seed, rid):
    """Draws u_first .. u_(first + count - 1) below N."""
    return draw_trace(first, count, N, seed, rid)[0]


@lru_cache(maxsize=None)
def _picked(N, mp, seed, rid):
    """The first mp distinct values of the draw sequence, in draw order, or None when the guard ends the replicate."""
    seq = np.zeros(0, dtype=np.uint64)
    while True:
        _, first = np.unique(seq, return_index=True)
        if len(first) >= mp:
            return tuple(int(x) for x in seq[np.sort(first)[:mp]])
        if len(seq) >= MAX_DRAWS:
            return None
        more = min(MAX_DRAWS - len(seq), max(64, 2 * mp))
        seq = np.concatenate([seq, draws(len(seq), more, N, seed, rid)])


def sample_positions(N, m, seed, rid):
    """(positions, complement): the picked positions, and whether they are the cells left OUT of the sample. m >= N:
    every position, not a complement. (None, False) when the guard ends the replicate."""
    N, m = int(N), int(m)
    if m >= N:
        return np.arange(N, dtype=np.int64), False
    mp = min(m, N - m)
    pk = _picked(N, mp, int(seed), int(rid))
    if pk is None:
        return None, False
    return np.asarray(pk, dtype=np.int64), mp != m


def batch_duplicate(N, m, seed, rid):
    """Whether two of the first min(64, m') draws (one batch of the kernel's lanes) are equal."""
    N, m = int(N), int(m)
    if m >= N:
        return False
    d = draws(0, min(64, m, N - m), N, int(seed), int(rid))
    return len(np.unique(d)) < len(d)


def sample_cells(nminus, row, m, seed, rid):
    """(n-, N+ copy numbers) of the sample, or None under the guard."""
    nminus = int(nminus)
    row = np.asarray(row, dtype=np.int64)
    N = nminus + len(row)
    pos, comp = sample_positions(N, m, seed, rid)
    if pos is None:
        return None
    if comp:
        keep = np.ones(N, dtype=bool)
        keep[pos] = False
        pos = np.flatnonzero(keep)
    return int((pos < nminus).sum()), row[pos[pos >= nminus] - nminus]


def sample_stats(nminus, row, m, seed, rid, bins, target=None):
    """ecdna_rep_stats_t of the sample (all zero under the guard)."""
    s = sample_cells(nminus, row, m, seed, rid)
    if s is None:
        return dict(cells=0, mean=0.0, entropy=0.0, frequency=0.0, ks=0.0, mean_rel=0.0, entropy_rel=0.0,
                    frequency_diff=0.0)
    return abc_stats.rep_stats(s[0], s[1], bins, target)


def sample_hist(nminus, row, m, seed, rid, bins):
    """The sample's histogram [bins] (bin 0 = N- cells, last bin = overflow; zero under the guard)."""
    s = sample_cells(nminus, row, m, seed, rid)
    h = np.zeros(bins, dtype=np.uint64)
    if s is not None:
        h += np.bincount(np.minimum(s[1], bins - 1), minlength=bins).astype(np.uint64)
        h[0] += np.uint64(s[0])
    return h


# --- described states: a population given by its summary, bin counters and row, never expanded -----------------------
# Download order: the nminus N- cells, the counters' cells k = 1..K ascending, then the row.

POSITION_LIMIT = 0xFFFFFFFF  # positions are u32 and 0xffffffff marks an empty table slot: N >= 2^32 - 1 is the guard
_ZERO = dict(cells=0, mean=0.0, entropy=0.0, frequency=0.0, ks=0.0, mean_rel=0.0, entropy_rel=0.0, frequency_diff=0.0)


def described_k(nminus, counters, row, pos):
    """Copy numbers of the positions `pos` of the state (nminus, counters[K], row): 0 for an N- cell, -1 for a position
    the counters and the row cannot account for. np.searchsorted on the inclusive prefix sums; nothing is expanded."""
    nminus = int(nminus)
    row = np.asarray(row, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    edges = nminus + np.cumsum(np.asarray(counters, dtype=np.uint64), dtype=np.uint64).astype(np.int64)
    row_from = int(edges[-1]) if len(edges) else nminus
    k = np.zeros(len(pos), dtype=np.int64)
    binned = (pos >= nminus) & (pos < row_from)
    k[binned] = np.searchsorted(edges, pos[binned], side="right") + 1  # the first counter whose prefix sum passes pos
    j = pos[pos >= row_from] - row_from
    kr = np.full(len(j), -1, dtype=np.int64)
    kr[j < len(row)] = row[j[j < len(row)]]
    k[pos >= row_from] = kr
    return k


def described_sample_cells(nminus, counters, row, m, seed, rid, nplus=None, table_slots=None):
    """(n-, N+ copy numbers) of the sample of m cells of a described state, the N+ cells in sample_cells' order; None
    under the guard. nplus: the summary's N+ cells (default: what the counters and the row hold); the row counts for
    min(nplus - sum(counters), len(row)) cells. The guard: N >= 2^32 - 1 with m < N, counters that hold more cells than
    the summary, a table of fewer than 2 * pow2ceil(m') slots (table_slots; None: as large as m' needs), 2^16 draws,
    and a position of the sample's making (picked, or walked for a complement) that nothing accounts for."""
    nminus, m = int(nminus), int(m)
    small = int(np.asarray(counters, dtype=np.uint64).sum()) if len(counters) else 0
    row = np.asarray(row, dtype=np.int64)
    nplus = small + len(row) if nplus is None else int(nplus)
    N = nminus + nplus
    if m < N and (N >= POSITION_LIMIT or small > nplus):
        return None
    row = row[:max(0, min(nplus - small, len(row)))]
    if m < N and table_slots is not None:
        mp = min(m, N - m)
        if table_slots < 2 * (1 << (mp - 1).bit_length() if mp > 1 else 1):
            return None
    pos, comp = sample_positions(N, m, seed, rid)
    if pos is None:
        return None
    if comp:
        keep = np.ones(N, dtype=bool)
        keep[pos] = False
        pos = np.flatnonzero(keep)
    k = described_k(nminus, counters, row, pos)
    if (k < 0).any():
        return None
    return int((pos < nminus).sum()), k[pos >= nminus]


def described_sample_stats(nminus, counters, row, m, seed, rid, bins, target=None, **kw):
    """ecdna_rep_stats_t of the sample of a described state (all zero under the guard)."""
    s = described_sample_cells(nminus, counters, row, m, seed, rid, **kw)
    return dict(_ZERO) if s is None else abc_stats.rep_stats(s[0], s[1], bins, target)


def described_sample_hist(nminus, counters, row, m, seed, rid, bins, **kw):
    """The sample's histogram [bins] of a described state (zero under the guard)."""
    s = described_sample_cells(nminus, counters, row, m, seed, rid, **kw)
    h = np.zeros(bins, dtype=np.uint64)
    if s is not None:
        h += np.bincount(np.minimum(s[1], bins - 1), minlength=bins).astype(np.uint64)
        h[0] += np.uint64(s[0])
    return h
