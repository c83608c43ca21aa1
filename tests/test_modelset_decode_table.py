"""CPU: the block tables of a model set's decode pass (spec_viterbi_amd/csrc/set_table.cpp, plain host
code) under AddressSanitizer + UBSan, through the stand-alone program
tests/cpp/test_set_decode_table.cpp: members of 0, 1, W - 1, W and W + 1 chosen rows at every workgroup
width, up to 65 entries; every block of the forward table (ceil(rows / W) x ranges blocks per entry) and
of the traceback table (build_set_row_table: one block per row) checked by brute force, and the refusal
of grids past 2^31 - 1.  Nothing is loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_set_decode_table")


def test_set_decode_table_under_asan():
    assert os.path.exists(BIN), "tests/cpp/test_set_decode_table not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
