"""ABC rejection on the GPU (ecdna_ssa_ctx_accept / ecdna_ssa_ctx_download_accept, added within ABI v13)
without a GPU: the header declares both calls with their argument lists, the library exports them, the ctypes mirrors
have the header's layout, the older blocks kept their sizes, the version is still 13, and both calls refuse a NULL
context with a message."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from ecdna_evo_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ecdna_ssa.h")
PARAMS_SIZE_V13 = 184  # sizeof(ecdna_ssa_params_t) as ABI v13 introduced it (LP64)


@pytest.fixture(scope="module")
def product_lib():
    from ecdna_evo_amd import engine

    return engine.lib()


def _declared(text, name):
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"include/ecdna_ssa.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_calls(product_lib):
    from ecdna_evo_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert _declared(text, "ecdna_ssa_ctx_accept") == ["ecdna_ssa_ctx* c", "const ecdna_ssa_accept_t* a"]
    assert _declared(text, "ecdna_ssa_ctx_download_accept") == [
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
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("FINAL", "SAMPLE", "SNAPSHOTS", "SNAPSHOT_SAMPLES", "PASSAGES", "PASSAGE_SAMPLES"):
        m = re.search(r"\bECDNA_ACCEPT_" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == getattr(abi, "ACCEPT_" + name), name


def test_accept_layouts_match_header(tmp_path):
    """sizeof and the field offsets from a compiled C probe against the ctypes mirrors; the older blocks did not move."""
    structs = (("ecdna_ssa_accept_t", abi.Accept, 48), ("ecdna_accept_threshold_t", abi.AcceptThreshold, 32))
    assert [f for f, _ in abi.Accept._fields_] == ["struct_size", "source", "n_thresholds", "list_threshold",
                                                   "thresholds", "timepoint_mask", "list_capacity", "reserved"]
    assert [f for f, _ in abi.AcceptThreshold._fields_] == ["ks", "mean_rel", "entropy_rel", "frequency_diff"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("{");']
    for cname, mirror, _ in structs:
        lines.append(f'printf("\\"{cname}\\": %zu, ", sizeof({cname}));')
        for f, _ in mirror._fields_:
            lines.append(f'printf("\\"{cname}.{f}\\": %zu, ", offsetof({cname}, {f}));')
    lines += ['printf("\\"passages\\": %zu, ", sizeof(ecdna_ssa_passages_t));',
              'printf("\\"ext\\": %zu, ", sizeof(ecdna_ssa_ext_t));',
              'printf("\\"stats\\": %zu, ", sizeof(ecdna_rep_stats_t));',
              'printf("\\"summary\\": %zu, ", sizeof(ecdna_rep_summary_t));',
              'printf("\\"params\\": %zu}\\n", sizeof(ecdna_ssa_params_t));', "return 0;}"]
    src = tmp_path / "accept_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "accept_layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
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
