"""The headline quad-ring kernel's unrolled block in the compiler's assembly (tools/diag_rdplace_check.py):
its LDS reads stand where the kept read placement puts them (diag_body.h block(), SVH_DIAG_RDPLACE = 1):
every two-step body's reads -- two constants, two quads and, every other body, the address group -- are
ONE run of consecutive instructions ahead of the body's counted wait, no other instruction between two
of them (at most two bodies of the 32 have the group read in a run of its own, behind a buffer's base
address); exactly 32 waits name lgkmcnt, one per body, and none waits for everything.  The order of the
other instantiations (SVH_DIAG_RDPLACE = 0), which has an address add between the reads of every other
body, fails the first of these.

Builds build/diag.dev.s by the Makefile's rule (about half a minute; build/ is ignored by git); skipped
where there is no hipcc.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def figures():
    made = subprocess.run(["make", "build/diag.dev.s"], cwd=ROOT, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout[-2000:] + made.stderr[-4000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import diag_rdplace_check
    finally:
        sys.path.pop(0)
    r = diag_rdplace_check.check(os.path.join(ROOT, "build", "diag.dev.s"))
    print(r)
    return r


def test_a_bodys_reads_are_one_run(figures):
    assert figures["bodies_other"] == 0 and figures["bodies_group_apart"] <= 2 and figures["bodies_one_run"] >= 30, figures
    assert figures["longest_run"] <= 5 and figures["reads_behind_last_wait"] == 0, figures


def test_one_wait_per_two_steps(figures):
    assert figures["waits"] == 32, figures


def test_no_wait_for_everything(figures):
    assert figures["zero_counts"] == 0, figures
