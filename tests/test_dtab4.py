"""CPU: the host layout of the diagonal plan's quad table (PipePlan::dtab4, runtime.cpp) through the
stand-alone program tests/cpp/test_dtab4.cpp, built with AddressSanitizer + UBSan: for small chain
models, dtab4 is the re-pairing {ea[c], ea[(c + 64) % NP], eb[c], eb[(c + 64) % NP]} of dtab2 with equal
float bits, for NP = 128 and 256, full position spaces and padded (+inf) columns.  Nothing is loaded
into Python and no GPU is touched."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_dtab4")


def test_dtab4_is_the_repairing_of_dtab2():
    assert os.path.exists(BIN), "tests/cpp/test_dtab4 not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
