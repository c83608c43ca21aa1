"""The headline quad-ring kernel's unrolled block in the compiler's assembly: the two-diagonal step
whose {F, c} register pair advances in place (diag_body.h step2, SVH_DIAG_S2PAIR = 1) is four packed
adds and no plain one per step, 256 v_pk_add_f32 and no v_add_f32 in the block of 64, and has no
register move: at most 4 v_mov_b32 in the whole block, none between a two-step body's wait and its
last v_cmpx.  The build that leaves the pair to the compiler (SVH_DIAG_S2PAIR = 0) has the same adds and
a v_mov_b32 in every step: it fails the move count (tools/diag_rdplace_check.py step2_figures()).

Builds build/diag.dev.s by the Makefile's rule and the other build beside it in build/s2pair0/ (about
half a minute each; build/ is ignored by git); skipped where there is no hipcc.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def figures_of(make_args, asm):
    made = subprocess.run(["make"] + make_args, cwd=ROOT, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout[-2000:] + made.stderr[-4000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import diag_rdplace_check
    finally:
        sys.path.pop(0)
    r = diag_rdplace_check.step2_figures(os.path.join(ROOT, asm))
    print(r)
    return r


@pytest.fixture(scope="module")
def kept():
    return figures_of(["build/diag.dev.s"], "build/diag.dev.s")


@pytest.fixture(scope="module")
def plain():
    return figures_of(["BUILD=build/s2pair0", "EXTRA_HIPFLAGS=-DSVH_DIAG_S2PAIR=0", "build/s2pair0/diag.dev.s"],
                      "build/s2pair0/diag.dev.s")


def test_adds_of_the_kept_step(kept):
    assert kept["checks"] == 64, kept
    assert kept["packed_adds"] == 256 and kept["plain_adds"] == 0, kept


def test_no_move_in_a_step(kept):
    assert kept["moves"] <= 4 and kept["moves_in_steps"] == 0, kept


def test_left_to_the_compiler_the_pair_has_its_moves(plain):
    assert plain["packed_adds"] == 256 and plain["plain_adds"] == 0, plain
    assert plain["moves"] >= 64 and plain["moves_in_steps"] > 4, plain  # (as built for the change: 67 and 44)
