"""GPU tests of the diagonal plan's speculation check and stream layout (diag.hip).

The existing diag tests cover lengths, the wrap, alphabets and models whose every row fails.  Here
rows fail on demand, at a chosen observation, beside rows that must not: a wave whose lanes failed
still refills the ring its workgroup's other waves read, and nothing of a failed row may leak into
the next launch.  The stream tests walk the lengths around the four-step address groups.

Rows that fail on demand: an MSV-shaped model (random_chain_hmm) whose M -> N weight (3 bits) is
dearer than N's self loop (< 1 bit).  For the symbol Z the M states emit almost for free and N
dearly (12 bits); for every other symbol it is the reverse.  A run of Z makes F grow faster than the
chain scores, so the check fl(A_F + x) < fl(X_FF + F) fires one or two observations later; a row
without Z cannot fail.  `spec_violations` restates the speculated recurrence and the check in numpy
(float32, the kernel's association) and fixes on the CPU which rows fail, at which observation and
on which diagonals; the GPU assertions are the exact fallback count and the oracle on every row.
"""
import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.helpers import bit_equal, first_mismatch, random_chain_hmm, random_seqs

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
Z = 0        # the symbol that makes a row fail
L = 150      # light rows: 3 ranges of 64 diagonals, 42 dummy positions
NP = 192
S = 4
LEN = 297    # observation 0, four blocks of 64 steps and a partial block of 40
INF = np.float32(np.inf)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def failing_model(seed=0, entry=None):
    """The model above; starts in N and in two light rows (so that observation 1 can fail).  entry =
    (p0, p1): only the light positions p0 .. p1-1 keep a payable N -> M term (60 bits elsewhere), so
    cheap scores enter the chain there alone and travel along their diagonals."""
    hmm = random_chain_hmm(L, S=S, seed=seed, start=(0, 5, 101))
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    w = hmm.trans_probs.copy()
    w[(cols == 0) & (rows != 0)] = np.float32(3.0)
    if entry is not None:
        pos = cols - 1
        w[(rows == 0) & (cols >= 1) & (cols <= L) & ~((pos >= entry[0]) & (pos < entry[1]))] = np.float32(60.0)
    hmm.trans_probs = w
    rng = np.random.default_rng(1000 + seed)
    em = np.asarray(hmm.emissions, np.float32).reshape(S, L + 2).copy()
    em[:, 1:L + 1] = rng.uniform(6.0, 8.0, size=(S, L)).astype(np.float32)
    em[:, 0] = np.float32(0.01)
    em[Z, 1:L + 1] = np.float32(0.001)
    em[Z, 0] = np.float32(12.0)
    hmm.emissions = em.reshape(np.asarray(hmm.emissions).shape)
    return hmm


def spec_violations(hmm, seq):
    """viol[t, p]: the check of observation t fires for light position p's score of t - 1, in the
    speculated run (F' = fl(X_FF + F) at every observation), float32 with the kernel's association:
    fl(A_F + x) < fl(X_FF + F), A_F = fl(e_N + w_MN), X_FF = fl(e_N + w_NN)."""
    n = hmm.states_num
    nl = n - 2
    em = np.asarray(hmm.emissions, np.float32).reshape(hmm.emit_num, n)
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    w = np.asarray(hmm.trans_probs, np.float32)
    w_nn = w[(rows == 0) & (cols == 0)][0]
    w_mn = w[(rows != 0) & (cols == 0)][0]
    w_nm = np.full(nl, INF, np.float32)
    w_ch = np.full(nl, INF, np.float32)
    for r, c, v in zip(rows, cols, w):
        if r == 0 and 1 <= c <= nl:
            w_nm[c - 1] = v
        elif 1 <= r <= nl and c == r + 1 and c <= nl:
            w_ch[c - 1] = v
    seq = np.asarray(seq, np.int64)
    x = np.full(nl, INF, np.float32)
    F = INF
    for c, v in zip(hmm.start_probabilities_cols.astype(np.int64), np.asarray(hmm.start_probabilities, np.float32)):
        if c == 0:
            F = np.float32(em[seq[0], 0] + v)
        elif 1 <= c <= nl:
            x[c - 1] = np.float32(em[seq[0], c] + v)
    viol = np.zeros((seq.size, nl), bool)
    for t in range(1, seq.size):
        o = seq[t]
        a_f = np.float32(em[o, 0] + w_mn)
        x_ff = np.float32(em[o, 0] + w_nn)
        fn = np.float32(x_ff + F)
        viol[t] = (a_f + x).astype(np.float32) < fn
        e = em[o, 1:nl + 1]
        ea = (e + w_nm).astype(np.float32)
        eb = (e + w_ch).astype(np.float32)
        prev = np.concatenate(([INF], x[:-1])).astype(np.float32)
        x = np.minimum((eb + prev).astype(np.float32), (ea + F).astype(np.float32))
        F = fn
    return viol


def first_violation(viol):
    t = np.nonzero(viol.any(axis=1))[0]
    return int(t[0]) if t.size else None


def violating_ranges(viol):
    """Ranges (of 64 diagonals) that hold a failing lane: the score of position p at observation
    t - 1 sits on diagonal (p - (t - 1)) mod NP."""
    t, p = np.nonzero(viol)
    return set((((p - (t - 1)) % NP) // 64).tolist())


def clean_seq(length, seed):
    return np.random.default_rng(seed).integers(1, S, size=length).astype(np.uint64)


def seq_failing_at(hmm, length, T, seed):
    """A sequence whose first violation is at observation T exactly (a run of Z ending before T)."""
    base = clean_seq(length, seed)
    for start in (T - 1, T - 2, T - 3):
        for run in (1, 2, 3):
            if start < 0 or start + run > T:
                continue
            seq = base.copy()
            seq[start:start + run] = Z
            if first_violation(spec_violations(hmm, seq)) == T:
                return seq
    raise AssertionError(f"no run of Z puts the first violation at observation {T}")


def run_twice(hmm, seqs):
    model = svh.DeviceModel(hmm, kernel=DIAG)
    b = model.batch(seqs)
    assert b.plan()["kernel"] == DIAG
    out = []
    for _ in range(2):
        b.run()
        s, best = b.read()
        out.append(([np.array(r, copy=True) for r in s], np.array(best, copy=True), b.fallbacks()))
    b.close()
    model.close()
    return out


def check(hmm, seqs, expect_fail):
    """CPU: exactly the rows of expect_fail violate.  GPU: that many rows fell back, every row equals
    the oracle, and a second run of the same batch gives the same (no state survives a launch)."""
    failing = {q for q, s in enumerate(seqs) if spec_violations(hmm, s).any()}
    assert failing == set(expect_fail), (failing, expect_fail)
    (s1, b1, fb1), (s2, b2, fb2) = run_twice(hmm, seqs)
    assert fb1 == len(expect_fail) and fb2 == fb1, (fb1, fb2, expect_fail)
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    for q in range(len(seqs)):
        assert bit_equal(s1[q], refs[q]), (q, first_mismatch(s1[q], refs[q]))
        assert bit_equal(s2[q], s1[q]), (q, first_mismatch(s2[q], s1[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert b1[q] == ref_best and b2[q] == ref_best, (q, b1[q], b2[q], ref_best)


@pytest.fixture(scope="module")
def model():
    return failing_model(seed=1)


@pytest.mark.parametrize("slot", [0, 3])
def test_mixed_workgroup_one_wave_fails_in_block0(model, slot):
    """Four rows in one workgroup; the row of wave `slot` fails in block 0 (observation 10), the other
    three run four blocks and a tail on ring groups the failing wave helped refill."""
    seqs = [clean_seq(LEN, 10 + q) for q in range(4)]
    seqs[slot] = seq_failing_at(model, LEN, 10, 20 + slot)
    check(model, seqs, [slot])


@pytest.mark.parametrize("T", [1, 64, 65, 4 * 64 + 20, LEN - 1])
def test_first_violation_position(model, T):
    """The first violation at step 1, at the last step of a full block, at the first of the next, inside
    the partial last block and at the row's last observation."""
    seqs = [clean_seq(LEN, 30 + q) for q in range(4)]
    seqs[1] = seq_failing_at(model, LEN, T, 40 + T)
    check(model, seqs, [1])


def test_violations_in_one_range_only():
    """N -> M payable at eight positions only: the cheap scores that fail ride a few neighbouring
    diagonals, all of range 1 or all of range 2, none of range 0."""
    hmm = failing_model(seed=2, entry=(100, 108))
    bad = clean_seq(LEN, 50)
    bad[130:133] = Z
    viol = spec_violations(hmm, bad)
    ranges = violating_ranges(viol)
    assert len(ranges) == 1 and 0 not in ranges, ranges
    seqs = [clean_seq(LEN, 51), clean_seq(LEN, 52), bad, clean_seq(LEN, 53)]
    check(hmm, seqs, [2])


@pytest.mark.parametrize("nseq,bad", [(5, 4), (2, 1), (1, 0)])
def test_idle_waves_and_narrow_workgroups(model, nseq, bad):
    """Five rows (the failing row alone with three idle waves in the second workgroup), two rows (two
    waves per workgroup) and one row (one wave)."""
    seqs = [clean_seq(LEN - 7 * q, 60 + q) for q in range(nseq)]
    seqs[bad] = seq_failing_at(model, len(seqs[bad]), 70, 70 + nseq)
    check(model, seqs, [bad])


LAYOUT_LENGTHS = list(range(2, 10)) + list(range(63, 71))


def test_stream_layout_lengths_plain():
    """Rows of 2..9 and 63..70 observations (the address stream is read four steps at a time, a block is
    64 steps), no row falls back."""
    hmm = random_chain_hmm(L, S=6, seed=7, n_from_m=False)
    seqs = random_seqs(6, LAYOUT_LENGTHS, seed=8)
    (s, b, fb), _ = run_twice(hmm, seqs)
    assert fb == 0
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    for q in range(len(seqs)):
        assert bit_equal(s[q], refs[q]), (q, first_mismatch(s[q], refs[q]))


def test_stream_layout_lengths_sx():
    """The same lengths on the sx model of test_diag_chain_variants (N -> C: the X_SF stream)."""
    hmm = random_chain_hmm(600, S=12, seed=11, sx=True)
    hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))
    hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(hmm.states_num - 1))
    hmm.trans_probs = np.append(hmm.trans_probs, np.float32(3.5))
    hmm.trans_num += 1
    seqs = random_seqs(12, LAYOUT_LENGTHS, seed=12)
    (s, b, fb), _ = run_twice(hmm, seqs)
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    for q in range(len(seqs)):
        assert bit_equal(s[q], refs[q]), (q, first_mismatch(s[q], refs[q]))
