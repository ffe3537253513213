"""Independent restatements of the host library's sampling (tests/test_host.py), which the CLI test and the
subsample law's tests use too."""


def _philox(ctr, key):
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = list(ctr)
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
    return c


def subsample_py(nplus, nminus, nb, seed, rid, k):
    """Independent restatement of host::subsample (Floyd's algorithm over cell positions)."""
    N = nminus + len(nplus)
    if nb >= N:
        return list(nplus), nminus
    words, blk = [], 0

    def nxt():
        nonlocal blk
        if not words:
            words.extend(_philox([k, 0x80000000 | blk, rid & 0xFFFFFFFF, rid >> 32], [seed & 0xFFFFFFFF, seed >> 32]))
            blk += 1
        return words.pop(0)

    def below(n):
        m = nxt() * n
        if (m & 0xFFFFFFFF) < n:
            thr = (2**32 - n) % n
            while (m & 0xFFFFFFFF) < thr:
                m = nxt() * n
        return m >> 32

    pick = set()
    for j in range(N - nb, N):
        t = below(j + 1)
        pick.add(j if t in pick else t)
    out = [nplus[i - nminus] for i in sorted(pick) if i >= nminus]
    return out, sum(1 for i in pick if i < nminus)
