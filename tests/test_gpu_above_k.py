"""Copy numbers near and above the bin store's K on the bin stepper's event path, bit for bit against
the oracle.

The K = 32 stepper treats such cells apart: a division of 65 .. 96 bits (k 33 .. 48) takes the event's third base
word (w3 and both spares) when two spares are in hand and a Philox block otherwise, larger ones always take blocks, and
a picked cell above K is read from the large-k row in HBM inside the event. The cases start from cells at 32, 33, 48, 49
(n = 64, 66, 96, 98) and mixed populations, with and without a pool of N- cells (which fills the spare stack), under
every segregation rule with draws and both processes, and run under both instruction schedules and under a rotation
that parks replicates every iteration or every eighth on one and on eight workgroups, so that the spare stack and the
large-k row cross lanes in every state. The event hash on (the runtime-flags instances) and off (the bench's)."""
import functools

import numpy as np
import pytest

from ecdna_evo_amd import abi
from support.gpu import _compare

H = abi.FLAG_EVENT_HASH
BD_RATES = (1.0, 1.5, 0.3, 0.3)
PB_RATES = (1.0, 1.2, 0.0, 0.0)

INITS = [
    ("k32", {32: 4}),
    ("k33", {33: 4}),
    ("k48", {48: 4}),
    ("k49", {49: 4}),
    ("k40_ones", {40: 2, 1: 50}),
    ("mixed_nminus", {0: 200, 1: 20, 20: 3, 36: 2, 44: 2}),  # an N- pool: N- events keep two spares in hand
]
SEGS = [("bin", abi.SEG_BINOMIAL), ("nouneven", abi.SEG_BINOMIAL_NO_UNEVEN), ("nonminus", abi.SEG_BINOMIAL_NO_NMINUS)]


def _specs():
    out = {}
    for i, (iname, init) in enumerate(INITS):
        for s, (sname, seg) in enumerate(SEGS):
            bd = (i + s) % 2 == 0
            hash_ = H if (3 * i + s) % 4 < 2 else 0
            out[f"{iname}_{sname}_{'bd' if bd else 'pb'}_h{int(bool(hash_))}"] = abi.RunSpec(
                seed=300 + 3 * i + s, process=abi.BIRTH_DEATH if bd else abi.PURE_BIRTH, segregation=seg,
                rates=(BD_RATES if bd else PB_RATES,), init=init, n_replicates=640, max_cells=1500, bin_kmax=32,
                flags=abi.FLAG_BIN_STORE | hash_)
    # no N- cell ever (none at the start, none from uneven splits) and no death: nothing pushes a spare, nsp stays 0
    out["no_spares_pb_h1"] = abi.RunSpec(seed=330, process=abi.PURE_BIRTH, segregation=abi.SEG_BINOMIAL_NO_NMINUS,
                                         rates=(PB_RATES,), init={40: 3, 34: 2}, n_replicates=640, max_cells=1500,
                                         bin_kmax=32, flags=abi.FLAG_BIN_STORE | H)
    # K = 64 with u16 counters: cells of k 33 .. 48 are binned here, and their divisions keep the Philox block loop
    out["k64_u16_bd_h0"] = abi.RunSpec(seed=331, process=abi.BIRTH_DEATH, rates=(BD_RATES,), init={0: 100, 48: 4, 70: 2},
                                       n_replicates=640, max_cells=1500, bin_kmax=64, flags=abi.FLAG_BIN_STORE)
    # a large-k row of six cells: divisions of large picks whose daughters stay above K stop with the capacity error
    out["big_cap_bd_h1"] = abi.RunSpec(seed=332, process=abi.BIRTH_DEATH, rates=(BD_RATES,), init={48: 4},
                                       n_replicates=640, max_cells=1500, bin_kmax=32, big_cap=6,
                                       flags=abi.FLAG_BIN_STORE | H)
    return out


SPECS = _specs()

# (ECDNA_SSA_SCHED, ECDNA_SSA_ROTATE, ECDNA_SSA_ROT_TICK, ECDNA_SSA_MAX_BLOCKS); the rotation parks whenever one
# replicate waits (ECDNA_SSA_ROT_PARK_MIN = 1)
LAUNCHES = [(sched, "0", None, None) for sched in ("2", "1")] + [
    (sched, "1", tick, blocks) for sched in ("2", "1") for tick in ("0", "3") for blocks in ("1", "8")]


@functools.lru_cache(maxsize=None)
def _cpu(name):
    import oracle

    oracle.build()
    return oracle.run(SPECS[name], mode="philox", want_rows=True)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_cases_reach_cells_above_k_and_above_48(name):
    """From the oracle alone, before any GPU run: every case ends with cells above its K in some replicate (so cells
    of the large-k row were there to be picked: every cell is picked with equal probability, and the runs make
    hundreds of thousands of picks) and with cells above 48 (so divisions of more than 96 bits took the general path)
    and in 33 .. 48 (65 .. 96 bits: the third word's range)."""
    cpu = _cpu(name)
    spec = SPECS[name]
    top = np.zeros(len(cpu.summaries), dtype=np.int64)
    mid = 0
    for i in range(len(top)):
        r = np.asarray(cpu.row(i))
        if len(r):
            top[i] = r.max()
            mid += int(((r > 32) & (r <= 48)).sum())
    if name.startswith("big_cap"):  # its replicates stop early, at the capacity error
        s = cpu.summaries
        assert (s["error"] == abi.REP_ERR_CELL_CAP).sum() > len(s) // 2
        assert (s["stop_reason"][s["error"] == abi.REP_ERR_CELL_CAP] == abi.STOP_ERROR).all()
    else:
        assert (top > 48).sum() >= 1, name
    assert (top > spec.bin_kmax).sum() >= 1, name
    assert mid >= 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SPECS))
def test_gpu_above_k_matches_oracle(name, engine_mod, oracle_mod, monkeypatch):
    spec = SPECS[name]
    cpu = _cpu(name)
    monkeypatch.setenv("ECDNA_SSA_ROT_PARK_MIN", "1")
    for sched, rotate, tick, blocks in LAUNCHES:
        monkeypatch.setenv("ECDNA_SSA_SCHED", sched)
        monkeypatch.setenv("ECDNA_SSA_ROTATE", rotate)
        for key, val in (("ECDNA_SSA_ROT_TICK", tick), ("ECDNA_SSA_MAX_BLOCKS", blocks)):
            if val is None:
                monkeypatch.delenv(key, raising=False)
            else:
                monkeypatch.setenv(key, val)
        _compare(engine_mod.run(spec, want_rows=True), cpu,
                 f"{name}/sched{sched}/rot{rotate}/tick{tick}/blocks{blocks}")
