"""ABC thresholds on the GPU (ecdna_ssa_ctx_select / ecdna_ssa_ctx_select_digits, added within ABI v13)
without a GPU: the header declares both calls with their argument lists, the library exports them, the ctypes mirror has
the header's layout, the older blocks kept their sizes, the version is still 13, both calls refuse a NULL context with a
message, and the header states select mapping v1 and its consequence for ecdna_ssa_ctx_accept."""
import ctypes as C
import re

from ecdna_evo_amd import abi
from support.abi import HEADER, PARAMS_SIZE_V13, declared, header_text, layout, product_lib  # noqa: F401 (fixture)


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_select") == [
        "ecdna_ssa_ctx* c", "const ecdna_ssa_select_t* s", "uint64_t* out_population", "uint64_t* out_ranks",
        "double* out_values", "uint64_t* out_counts_le"]
    assert declared("ecdna_ssa_ctx_select_digits") == [
        "ecdna_ssa_ctx* c", "uint32_t source", "uint64_t timepoint_mask", "uint32_t pass", "uint32_t n_prefixes",
        "const uint64_t* prefixes", "uint64_t* out_hist"]
    for name in ("ecdna_ssa_ctx_select", "ecdna_ssa_ctx_select_digits"):
        assert hasattr(product_lib, name) and name in engine.EXPORTS
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_the_header_states_the_select_mapping_and_its_consequence():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Select mapping v1", "0x7FF8000000000000", "NaN sorts above +inf",
                   "the k-th smallest of the M keys", "> k on a tie", "value = +inf and counts_le = M",
                   "accepts exactly counts_le_x(k) replicates, and no smaller threshold accepts k or more",
                   "k = max(1, (uint64)ceil(f (double)M))", "Shards' arrays sum to the whole run's"):
        assert phrase in text, phrase
    assert "select mapping v1). A context that never calls them allocates and launches nothing new" in text


def test_select_layout_matches_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirror; the older blocks did not move."""
    assert [f for f, _ in abi.Select._fields_] == ["struct_size", "source", "timepoint_mask", "n_ranks", "reserved",
                                                   "ranks", "fractions"]
    got = layout(tmp_path, {"select": ("ecdna_ssa_select_t", [f for f, _ in abi.Select._fields_]),
                            "accept": "ecdna_ssa_accept_t", "threshold": "ecdna_accept_threshold_t",
                            "passages": "ecdna_ssa_passages_t", "ext": "ecdna_ssa_ext_t", "stats": "ecdna_rep_stats_t",
                            "summary": "ecdna_rep_summary_t", "params": "ecdna_ssa_params_t"})
    assert got["select"] == C.sizeof(abi.Select) == 40
    for f, _ in abi.Select._fields_:
        assert got[f"select.{f}"] == getattr(abi.Select, f).offset, f
    assert got["accept"] == C.sizeof(abi.Accept) == 48 and got["threshold"] == C.sizeof(abi.AcceptThreshold) == 32
    assert got["passages"] == C.sizeof(abi.Passages) == 24
    assert got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["stats"] == abi.STATS_DTYPE.itemsize == 64 and got["summary"] == abi.SUMMARY_DTYPE.itemsize == 88
    assert got["params"] == C.sizeof(abi.Params) == PARAMS_SIZE_V13  # ecdna_ssa_params_t did not grow


def test_both_calls_refuse_a_null_context(product_lib):
    ranks = (C.c_uint64 * 1)(1)
    s = abi.Select(struct_size=C.sizeof(abi.Select), source=abi.ACCEPT_FINAL, n_ranks=1)
    s.ranks = C.cast(ranks, C.POINTER(C.c_uint64))
    assert product_lib.ecdna_ssa_ctx_select(None, C.byref(s), None, None, None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    prefixes = (C.c_uint64 * 4)()
    hist = (C.c_uint64 * (4 * 256))()
    assert product_lib.ecdna_ssa_ctx_select_digits(None, abi.ACCEPT_FINAL, 0, 0, 1, prefixes, hist) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
