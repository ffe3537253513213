"""What the tests of the C ABI share: the header's text and declarations, the product library, and the compiled C probe
of the header's struct layout."""
import ctypes
import json
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(REPO, "include", "ecdna_ssa.h")
PARAMS_SIZE_V13 = 184  # sizeof(ecdna_ssa_params_t) as ABI v13 introduced it (LP64)


def header_text():
    """include/ecdna_ssa.h without its comments."""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def declared(name, returns="int"):
    """The parameters of the header's declaration of `name`, one string each, blanks squeezed."""
    m = re.search(returns + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header_text())
    assert m, f"include/ecdna_ssa.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.fixture(scope="module")
def product_lib():
    """The library with the package's signatures (engine.lib(): one handle per process)."""
    from ecdna_evo_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return engine.lib()


def raw_lib():
    """A fresh handle of the library without signatures, for calls that pass what the package's argtypes refuse."""
    from ecdna_evo_amd import engine

    return ctypes.CDLL(engine.LIB_PATH)


def layout(tmp_path, structs, values=None):
    """A compiled C probe of the header. structs: {key: C type, or (C type, fields)}; values: {key: C int expression}.
    Returns {key: sizeof, "key.field": offsetof, ..., key: value}."""
    items = []  # (key, printf format, C expression)
    for key, what in structs.items():
        ctype, fields = (what, ()) if isinstance(what, str) else what
        items.append((key, "%zu", f"sizeof({ctype})"))
        items += [(f"{key}.{f}", "%zu", f"offsetof({ctype}, {f})") for f in fields]
    items += [(key, "%d", f"(int)({expr})") for key, expr in (values or {}).items()]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){", 'printf("{");']
    lines += [f'printf("{", " if i else ""}\\"{key}\\": {fmt}", {expr});' for i, (key, fmt, expr) in enumerate(items)]
    lines += ['printf("}\\n");', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    return json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
