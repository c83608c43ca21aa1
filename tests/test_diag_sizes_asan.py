"""CPU: the diagonal path variant's record-size helpers and the offset sums Batch::load forms from
them, under AddressSanitizer + UBSan (tests/cpp/test_diag_sizes_asan.cpp, a stand-alone program)."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_diag_sizes_asan")


def test_diag_path_sizes_under_asan():
    assert os.path.exists(BIN), "tests/cpp/test_diag_sizes_asan not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
