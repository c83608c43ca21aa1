"""CPU: the pass resolver (spec_viterbi_amd/csrc/dispatch.cpp, plain host code) under
AddressSanitizer + UBSan, through the stand-alone program tests/cpp/test_dispatch.cpp: every
consistent capability record x kernel preference x rows x paths x level x scratch by brute force --
the result is total and deterministic, no pipelined or diagonal step kernel without scratch, no
pipelined plan without a chain plan, path records consistent with the step kernel, a chunk route
exactly at level >= 2 on built products -- and the named cases of DESIGN.md 5c / 5l / 5n.  Nothing is
loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp", "test_dispatch")


def test_dispatch_under_asan():
    assert os.path.exists(BIN), "tests/cpp/test_dispatch not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BIN], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "ok" in r.stdout, r.stdout
