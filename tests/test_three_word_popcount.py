"""The bin stepper's branch-free segregation popcount over the event's own stream words (w3 and up to two spares:
divisions of up to 96 bits, ecdna-evo_amd/csrc/ssa_device.hpp popcount_base_words) against the word-by-word first loop
of WordStream::binomial_half_with, on the CPU."""
import subprocess

from support import native


@native.needs_hipcc
def test_three_word_popcount_matches_the_word_loop(tmp_path_factory):
    """Every n in 1 .. 96 with 0, 1 and 2 spares in hand, over the eight all-ones / all-zero word combinations and
    2,000 random word triples each: where the words in hand hold all of n (n <= 32 + 32 * nsp; the stepper calls it for
    65 <= n <= 96 with two spares) the value equals the loop's count and the loop has consumed all of n at stream
    position (n + 63) >> 5; elsewhere the loop leaves bits for the Philox blocks. The value ignores every bit past the
    n-th (tests/native/three_word_popcount_check.cpp)."""
    exe = native.build(tmp_path_factory, "three_word_popcount_check", sanitize=False)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    fields = dict(kv.split("=") for kv in out.stdout.split())
    # fast cases: n <= 32 (nsp 0), 64 (nsp 1), 96 (nsp 2), 2,008 word triples each
    assert int(fields["cases"]) == (32 + 64 + 96) * 2008
    assert int(fields["mismatches"]) == 0
