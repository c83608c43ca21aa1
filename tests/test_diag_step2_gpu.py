"""GPU parity of the two-diagonal step whose {F, c} register pair advances in place (diag_body.h step2,
SVH_DIAG_S2PAIR) and of the row's last, partial block (tail()): one asm statement adds the pair and
takes the sink's minimum in a fixed register pair, the speculation check compares against the new F'
in it, and every row ends in a tail, a rolled loop over the same step, whose stream buffer is only
partly written.

A small two-range model (200 light states: NP = 256, two ranges of 128 positions), SVH_DIAG_SM=2 and
SVH_DIAG_LOADER=1 forced; five rows of different lengths per batch, four of them the step waves of one
workgroup, which end in different blocks and tails.  A row of L observations runs L - 1 steps.  The
step counts are 1 .. 5 and 63 (block 0 is itself the tail) and the same offsets behind 64 steps (a
tail behind one full block), 128 (two), 320 (the ring's five groups once around) and 384 (the mirror's
second turn), and one tail of 43 steps, the headline's.  Each under SVH_DIAG_QUAD=1 and =0 (the quad
and the plane layout), with the same fallback count; some under SVH_DIAG_SM=1 (the one-diagonal tail);
one model whose sink takes a term from the feeder (X_SF); and models whose feeder takes its light term,
so that the check fires and rows are re-run.  Scores and best states are bit-exact with the oracle.
"""
import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.helpers import bit_equal, first_mismatch, random_chain_hmm, random_seqs

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
TAIL_STEPS = (1, 2, 3, 4, 5, 63)
LENGTHS = [base + d + 1 for base in (0, 64, 128, 320, 384) for d in TAIL_STEPS] + [64 + 43 + 1]
LENGTHS_SM1 = [base + d + 1 for base in (0, 64, 320) for d in (1, 5, 63)] + [64 + 43 + 1]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


@pytest.fixture(scope="module")
def hmm():
    return random_chain_hmm(200, S=6, seed=2000, n_from_m=False)


def rows_of(L):
    return [L, 1, L + 64, 3 * L + 1, max(1, L - 3)]


def run(monkeypatch, hmm, seqs, sm=2, quad=None):
    monkeypatch.setenv("SVH_DIAG_SM", str(sm))
    monkeypatch.setenv("SVH_DIAG_LOADER", "1")
    if quad is None:
        monkeypatch.delenv("SVH_DIAG_QUAD", raising=False)
    else:
        monkeypatch.setenv("SVH_DIAG_QUAD", "1" if quad else "0")
    model = svh.DeviceModel(hmm, kernel=DIAG)
    b = model.batch(seqs)
    plan = b.plan()
    assert plan["kernel"] == DIAG and plan["diag_sm"] == sm, plan
    if quad is not None:
        assert plan["diag_quad"] == (1 if quad else 0), plan
    b.run()
    s, best = b.read()
    fb = b.fallbacks()
    b.close()
    model.close()
    return s, best, fb


def oracle_check(hmm, seqs, scores, best, refs=None):
    refs = oracle.viterbi_batch(hmm, seqs)[0] if refs is None else refs
    for q in range(len(seqs)):
        assert bit_equal(scores[q], refs[q]), (q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (q, best[q], ref_best)
    return refs


@pytest.mark.parametrize("L", LENGTHS)
def test_step2_tails_quad_and_planes(monkeypatch, hmm, L):
    seqs = random_seqs(6, rows_of(L), seed=L)
    s, best, fb = run(monkeypatch, hmm, seqs, quad=True)
    refs = oracle_check(hmm, seqs, s, best)
    sp, bestp, fbp = run(monkeypatch, hmm, seqs, quad=False)
    oracle_check(hmm, seqs, sp, bestp, refs)
    assert fb == fbp


@pytest.mark.parametrize("L", LENGTHS_SM1)
def test_one_diagonal_tails(monkeypatch, hmm, L):
    seqs = random_seqs(6, rows_of(L), seed=L)
    s, best, _ = run(monkeypatch, hmm, seqs, sm=1)
    oracle_check(hmm, seqs, s, best)


@pytest.mark.parametrize("quad", [True, False])
def test_step2_sink_fed_by_feeder(monkeypatch, quad):
    """S fed by N (the X_SF term of step2: the third minimum of the sink partial), S = 12."""
    hmm = random_chain_hmm(200, S=12, seed=2001, n_from_m=False)
    hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))  # N -> C
    hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(hmm.states_num - 1))
    hmm.trans_probs = np.append(hmm.trans_probs, np.float32(3.5))
    hmm.trans_num += 1
    seqs = random_seqs(12, rows_of(64 + 43 + 1), seed=12)
    s, best, _ = run(monkeypatch, hmm, seqs, quad=quad)
    oracle_check(hmm, seqs, s, best)


def test_step2_check_fires_rows_rerun(monkeypatch):
    """Models whose feeder row takes its light term (M -> N free): the check, against the pair's F', fails,
    the rows are re-run in the launch and every score matches the oracle."""
    total_fb = 0
    for seed in range(8):
        hmm = random_chain_hmm(300 if seed < 6 else 700, S=8, seed=seed)
        rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
        probs = hmm.trans_probs.copy()
        probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
        hmm.trans_probs = probs
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        s, best, fb = run(monkeypatch, hmm, seqs)
        total_fb += fb
        oracle_check(hmm, seqs, s, best)
    assert total_fb > 0
