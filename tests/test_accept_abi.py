"""ABC rejection on the GPU (ecdna_ssa_ctx_accept / ecdna_ssa_ctx_download_accept, added within ABI v13)
without a GPU: the header declares both calls with their argument lists, the library exports them, the ctypes mirrors
have the header's layout, the older blocks kept their sizes, the version is still 13, and both calls refuse a NULL
context with a message."""
import ctypes as C
import re

from ecdna_evo_amd import abi
from support.abi import HEADER, PARAMS_SIZE_V13, declared, header_text, layout, product_lib  # noqa: F401 (fixture)


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = header_text()
    assert declared("ecdna_ssa_ctx_accept") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_t* a"]
    assert declared("ecdna_ssa_ctx_download_accept") == [
        "ecdna_ssa_ctx* c", "uint64_t* out_counts", "uint32_t* out_mask", "uint64_t* out_n_accepted",
        "uint64_t* out_ids", "ecdna_rep_stats_t* out_list_stats"]
    for name in ("ecdna_ssa_ctx_accept", "ecdna_ssa_ctx_download_accept"):
        assert hasattr(product_lib, name) and name in engine.EXPORTS
    # additive: the version is v13's
    assert re.search(r"#define ECDNA_SSA_ABI_VERSION 13\b", text) and abi.ABI_VERSION == 13
    assert product_lib.ecdna_ssa_abi_version() == 13


def test_the_header_states_the_acceptance_rule():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("Acceptance mapping v1", "A distance equal to its threshold passes",
                   "A NaN distance fails unless the threshold is +inf", "every participating phase"):
        assert phrase in text, phrase


def test_the_source_constants_are_the_headers():
    text = header_text()
    for name in ("FINAL", "SAMPLE", "SNAPSHOTS", "SNAPSHOT_SAMPLES", "PASSAGES", "PASSAGE_SAMPLES"):
        m = re.search(r"\bECDNA_ACCEPT_" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == getattr(abi, "ACCEPT_" + name), name


def test_accept_layouts_match_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirrors; the older blocks did not move."""
    structs = (("ecdna_ssa_accept_t", abi.Accept, 48), ("ecdna_accept_threshold_t", abi.AcceptThreshold, 32))
    assert [f for f, _ in abi.Accept._fields_] == ["struct_size", "source", "n_thresholds", "list_threshold",
                                                   "thresholds", "timepoint_mask", "list_capacity", "reserved"]
    assert [f for f, _ in abi.AcceptThreshold._fields_] == ["ks", "mean_rel", "entropy_rel", "frequency_diff"]
    got = layout(tmp_path, {**{cname: (cname, [f for f, _ in mirror._fields_]) for cname, mirror, _ in structs},
                            "passages": "ecdna_ssa_passages_t", "ext": "ecdna_ssa_ext_t", "stats": "ecdna_rep_stats_t",
                            "summary": "ecdna_rep_summary_t", "params": "ecdna_ssa_params_t"})
    for cname, mirror, size in structs:
        assert got[cname] == C.sizeof(mirror) == size, cname
        for f, _ in mirror._fields_:
            assert got[f"{cname}.{f}"] == getattr(mirror, f).offset, (cname, f)
    assert got["passages"] == C.sizeof(abi.Passages) == 24
    assert got["ext"] == C.sizeof(abi.Ext) == 24
    assert got["stats"] == abi.STATS_DTYPE.itemsize == 64 and got["summary"] == abi.SUMMARY_DTYPE.itemsize == 88
    assert got["params"] == C.sizeof(abi.Params) == PARAMS_SIZE_V13  # ecdna_ssa_params_t did not grow


def test_both_calls_refuse_a_null_context(product_lib):
    thr = (abi.AcceptThreshold * 1)(abi.AcceptThreshold(1.0, 1.0, 1.0, 1.0))
    a = abi.Accept(struct_size=C.sizeof(abi.Accept), source=abi.ACCEPT_FINAL, n_thresholds=1)
    a.thresholds = C.cast(thr, C.POINTER(abi.AcceptThreshold))
    assert product_lib.ecdna_ssa_ctx_accept(None, C.byref(a)) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
    assert product_lib.ecdna_ssa_ctx_download_accept(None, None, None, None, None, None) == abi.E_INVALID
    assert product_lib.ecdna_ssa_last_error_message()
