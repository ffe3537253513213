"""The stand-alone programs of tests/native: built for the host alone, by default with the address and
undefined-behaviour sanitizers (any report ends them with an error), and run as processes of their own; they are never
loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc absent")


def build(tmp_path_factory, name, sanitize=True, extra=()):
    """tests/native/<name>.cpp as a program in a fresh directory; `extra`: further words of the hipcc line."""
    exe = os.path.join(str(tmp_path_factory.mktemp(name)), name)
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *(flags if sanitize else ()),
                    "-I", os.path.join(REPO, "ecdna-evo_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", name + ".cpp"), *extra, "-o", exe], check=True)
    return exe


def run(exe, *args, stdin=None):
    """The lines the program printed for `args` (and the text `stdin`)."""
    out = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-4000:]  # (no sanitizer report)
    return out.stdout.splitlines()


def _want_keep(keep, mask, sizes):
    """The keep store restated: one slice; the participating targets by distinct m1 in order of first appearance."""
    take = [p for p in range(len(sizes)) if mask == 0 or (mask >> p) & 1]
    order = list(dict.fromkeys(sizes[p] for p in take))
    groups = [(m, [p for p in take if sizes[p] == m]) for m in order]
    return 1, 1, max(min(m, keep - m) for m in order), [(0, len(groups))], groups


def _want_timepoints(keep, mask, sizes):
    """The timepoint store restated: slice t takes part when the mask names it, with one group of target t."""
    T = len(sizes)
    full = mask if mask else (1 << T) - 1
    take = [t for t in range(T) if (full >> t) & 1]
    slices, at = [], 0
    for t in range(T):
        slices.append((at, at + (t in take)))
        at += t in take
    return T, full, max(min(sizes[t], keep - sizes[t]) for t in take), slices, [(sizes[t], [t]) for t in take]
