"""TEST INFRASTRUCTURE ONLY — numpy restatement of thinning mapping v1 (include/ecdna_ssa.h), written from
the text of the mapping and not from the kernel.

The scored object is a kept sample: header {a, b} and cells[0 .. b), ascending true copy numbers (tests/keep_law.py).
Its population is N_k = a + b cells, the a N- cells first and then the cells. A target with m1 >= N_k measured cells is
scored on the whole kept sample (keep_law.rescored). Otherwise subsample mapping v1 is applied to that population with
m = m1, under the key the slice's own sample was drawn under (the run's seed; passage_law.seed_g for growth phase g), on
the stream whose field is the slice's own (0, or (s + 1) << 16 for snapshot s) with bit 29 set and the draw index d in
bits 10-15. The positions are snapshot_stats_law.sample_positions' with that field; the record is oracle/abc_stats.py's
of the thinned cells. The guard header {0xffffffff, 0xffffffff}, and the 2^16-draw guard, give the all-zero record.
"""
import numpy as np

import abc_stats
import keep_law as kl
import passage_law
import snapshot_stats_law as ssl

THIN_FLAG = 0x20000000
MAX_DRAW = 63


def field(d=0, snapshot=None):
    """The stream field of a thinning (counter word 1 without the tag 0xC0000000 and the block index): the slice's own
    field — 0 for the end of the run and for passage phases, (s + 1) << 16 for snapshot s — the thinning flag, and the
    draw index d."""
    assert 0 <= d <= MAX_DRAW
    own = 0 if snapshot is None else ssl.stream_field(snapshot)
    return own | THIN_FLAG | (d << 10)


def phase_key(seed, g=None):
    """The key of a slice: the run's seed, or the key of growth phase g of a passage context."""
    return int(seed) if g is None else passage_law.seed_g(seed, g)


def thinned(header, cells, m1, key, rid, d=0, snapshot=None):
    """(n-, N+ copy numbers) of the sample of m1 cells of the kept sample; the whole kept sample for m1 >= a + b; None
    under a guard."""
    if kl.is_guard(header):
        return None
    a, b = int(header[0]), int(header[1])
    row = np.asarray(cells, dtype=np.int64)[:b]
    N = a + b
    if m1 >= N:
        return a, row
    pos, comp = ssl.sample_positions(N, m1, key, rid, 0, field=field(d, snapshot))
    if pos is None:
        return None
    if comp:
        keep = np.ones(N, dtype=bool)
        keep[pos] = False
        pos = np.flatnonzero(keep)
    return int((pos < a).sum()), row[pos[pos >= a] - a]


def record(header, cells, m1, key, rid, bins, target, d=0, snapshot=None):
    """ecdna_rep_stats_t of the kept sample scored on m1 cells against `target` (all zero under a guard)."""
    s = thinned(header, cells, m1, key, rid, d, snapshot)
    if s is None:
        return dict(kl.ZERO_RECORD)
    return abc_stats.rep_stats(s[0], s[1], bins, target)
