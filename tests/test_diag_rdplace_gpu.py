"""GPU parity of the quad-ring kernels' read placement (diag_body.h block(), SVH_DIAG_RDPLACE): the body
reads the constants and the quads of two steps in one run, two steps ahead (four register slots of
constants instead of eight), the ring addresses eight.  What a change of the prefetch distances can
break is at the blocks' ends: a full block's prefetch into a block that is a tail or does not exist,
the register slots across a block boundary, the ring's wrap and the mirror's turn.  (The lengths also
cover the deeper distances, quads six steps ahead, of the placements that were measured and dropped.)

A small two-range model (200 light states: NP = 256, two ranges of 128 positions), SVH_DIAG_SM=2,
SVH_DIAG_LOADER=1 and SVH_DIAG_QUAD=1 forced; five rows of different lengths per batch, four of them
the step waves of one workgroup, which end in different blocks.  The row length L takes every value
from 65 (one full block of 64 steps and nothing behind it) to 65 + 6 + 2 (the deepest prefetch distance
the placements use, and the two steps being read), and the same offsets behind 129 (two blocks), 321
(five: the ring's five groups once around) and 385 (six: the mirror's second turn).  Scores and best
states are bit-exact with the oracle; the fallback count is the same batch's under SVH_DIAG_QUAD=0.
"""
import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.helpers import bit_equal, first_mismatch, random_chain_hmm, random_seqs

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
DEEPEST = 6  # steps ahead: the kept placement reads two ahead, the deepest one measured six
LENGTHS = [base + d for base in (65, 129, 321, 385) for d in range(DEEPEST + 3)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


@pytest.fixture(scope="module")
def hmm():
    return random_chain_hmm(200, S=6, seed=1900, n_from_m=False)


def run(monkeypatch, hmm, seqs, quad):
    monkeypatch.setenv("SVH_DIAG_SM", "2")
    monkeypatch.setenv("SVH_DIAG_LOADER", "1")
    monkeypatch.setenv("SVH_DIAG_QUAD", "1" if quad else "0")
    model = svh.DeviceModel(hmm, kernel=DIAG)
    b = model.batch(seqs)
    plan = b.plan()
    assert plan["kernel"] == DIAG and plan["diag_sm"] == 2 and plan["diag_quad"] == (1 if quad else 0), plan
    b.run()
    s, best = b.read()
    fb = b.fallbacks()
    b.close()
    model.close()
    return s, best, fb


@pytest.mark.parametrize("L", LENGTHS)
def test_rdplace_block_ends(monkeypatch, hmm, L):
    seqs = random_seqs(6, [L, 1, L + 64, 3 * L + 1, max(1, L - 3)], seed=L)
    s, best, fb = run(monkeypatch, hmm, seqs, True)
    refs = oracle.viterbi_batch(hmm, seqs)[0]
    for q in range(len(seqs)):
        assert bit_equal(s[q], refs[q]), (q, first_mismatch(s[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (q, best[q], ref_best)
    assert fb == run(monkeypatch, hmm, seqs, False)[2]
