"""CPU: the model sets' block table (spec_viterbi_amd/csrc/set_table.cpp, plain host code) under
AddressSanitizer + UBSan, through the stand-alone program tests/cpp/test_set_table.cpp: sets of 1,
64, 65 and 200 entries with members outside the set launch interleaved, every block of every grid
checked by brute force against the prefix table, the zero-range / zero-sequence / width guards and
the refusal of grids past 2^31 - 1.  Nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_set_table")


def test_set_table_under_asan():
    assert os.path.exists(BIN), "tests/cpp/test_set_table not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
