"""CPU: the diagonal plan's launch resolver (spec_viterbi_amd/csrc/diag_launch.cpp: which variant of the
kernel a launch is, its grid, workgroup and LDS) through the stand-alone program
tests/cpp/test_diag_launch.cpp, built with AddressSanitizer + UBSan: against
tests/golden/diag_launch_grid.jsonl, recorded from the launch code the resolver replaced, and the
invariants the launch relies on over the whole grid.  Nothing is loaded into Python and no GPU is touched."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_diag_launch")
GOLDEN = os.path.join(ROOT, "tests", "golden", "diag_launch_grid.jsonl")


def test_diag_resolve_matches_the_recorded_launches():
    assert os.path.exists(BIN), "tests/cpp/test_diag_launch not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
