"""The sampling passes' LDS plan as the library answers it (ecdna_dev_pass_lds, not part of the C ABI) and the restated
formulas that tests/test_pass_lds*.py share."""
import ctypes as C
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(REPO, "ecdna-evo_amd", "lib", "libecdna_ssa.so")
LDS_MAX = 65536
SUBSAMPLE, PASSAGE, SNAPSTATS = 0, 1, 2
BINS = (2, 64, 65, 257, 1025, 2047, 2048)
BAG_K = (0, 32, 64, 256)
M = (1, 63, 64, 65, 500, 2048, 2049, 4096)


@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(LIB):
        import __graft_entry__

        __graft_entry__.build()
    fn = C.CDLL(LIB).ecdna_dev_pass_lds
    fn.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                   C.POINTER(C.c_int)]
    fn.restype = C.c_int

    def call(which, bins, bag_k, m):
        waves, lds, in_lds = C.c_uint32(), C.c_uint64(), C.c_int()
        assert fn(which, bins, bag_k, m, C.byref(waves), C.byref(lds), C.byref(in_lds)) == 0
        return waves.value, lds.value, in_lds.value

    return call


def table_slots(m):
    p = 1
    while p < m:
        p <<= 1
    return 2 * p


def sort_slots(m):
    p = 64
    while p < m:
        p <<= 1
    return p


def waves_within(lds_of):
    """The first of 4, 2, 1 waves whose LDS fits, or one wave whatever it takes."""
    for nw in (4, 2, 1):
        if lds_of(nw) <= LDS_MAX or nw == 1:
            return nw, lds_of(nw)


def subsample_plan(bins, bag_k, m):
    return waves_within(lambda nw: bins * 8 + nw * (bins + bag_k + table_slots(m)) * 4) + (0,)


def passage_plan(bins, bag_k, m):
    return waves_within(lambda nw: nw * (bins + bag_k + table_slots(m) + sort_slots(m) // 2) * 4) + (0,)


def snapstats_plan(bins, m):
    slots = table_slots(m) if m else 0
    for in_lds in ((1, 0) if slots else (0,)):
        for nw in (4, 2, 1):
            lds = bins * (2 if in_lds else 1) * 8 + nw * (bins + slots) * 4
            if lds <= LDS_MAX or (nw == 1 and not in_lds):
                return nw, lds, in_lds
