"""GPU parity of the diagonal plan's two-diagonal variant (diag.hip, DM = 2): lane l of range r holds
diagonals 128 r + l and 128 r + 64 + l, ranges are 128 positions wide, the ring keeps an ea and an eb
plane per symbol, and the speculation check and the sink recurrence take the minimum of the lane's
two scores.

Every test but the AUTO one forces the variant (SVH_DIAG_SM=2, read when the model is created),
asserts that the batch's plan says so (`plan()["diag_sm"] == 2`) and compares scores and best states
bit-exact.  The shapes are the ones at which this kernel can go wrong: position spaces of one range
that wraps onto itself, an exactly full range, one position over (a range of 127 dummies) and a
64-wide-odd count (a padding half range); lengths around every block (64 steps) and prefetch
boundary; rows long enough for both diagonals of a lane to cross position 0 and the mirror's end.
As in test_diag_gpu.py, reference workloads assert that no row fell back (the exact re-run would hide
a wrong fast path) and models whose feeder row takes its light term assert that rows did.
"""
import hashlib

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.conftest import chmm, ess
from tests.helpers import (bit_equal, first_mismatch, from_hex, load_digests, load_golden, random_chain_hmm,
                           random_seqs)

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
CHAIN = _lib.SVH_KERNEL_CHAIN


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


@pytest.fixture
def sm2(monkeypatch):
    monkeypatch.setenv("SVH_DIAG_SM", "2")


def run(hmm, seqs, kernel=DIAG, want_sm=2):
    model = svh.DeviceModel(hmm, kernel=kernel)
    b = model.batch(seqs)
    plan = b.plan()
    if want_sm:
        assert plan["kernel"] == DIAG and plan["diag_sm"] == want_sm, plan
    b.run()
    s, best = b.read()
    fb = b.fallbacks() if kernel != CHAIN else 0
    b.close()
    model.close()
    return s, best, fb, plan


def assert_same(s1, b1, s2, b2):
    for q in range(len(s1)):
        assert bit_equal(s1[q], s2[q]), (q, first_mismatch(s1[q], s2[q]))
    assert np.array_equal(b1, b2)


def oracle_check(hmm, seqs, scores, best):
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    for q in range(len(seqs)):
        assert bit_equal(scores[q], refs[q]), (q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (q, best[q], ref_best)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 320])
def test_diag2_position_space_widths(sm2, L):
    """Light rows around the 64- and 128-wide boundaries: one range that wraps onto itself (L <= 128;
    L <= 64 leaves the second diagonal of every lane on dummies), an exactly full range (128, 256),
    one position over (129, 257: a range of 127 dummies), and 64-wide-odd counts (129, 130, 257,
    320: three or five ranges of 64 become two or three of 128, the last one half or wholly dummies).
    Rows longer than the position space, so every lane wraps many times."""
    hmm = random_chain_hmm(L, S=6, seed=200 + L, n_from_m=False)
    seqs = random_seqs(6, [3 * (L + 2) + 5, 700, 64], seed=L)
    s, b, fb, _ = run(hmm, seqs)
    assert fb == 0
    oracle_check(hmm, seqs, s, b)


@pytest.mark.parametrize("L", [1, 2, 3, 7, 8, 9, 63, 64, 65, 66, 127, 128, 129, 130])
def test_diag2_sequence_lengths(sm2, L):
    """Lengths around the block of 64 steps (the ring refill, the stream double buffer), the prefetch
    distances (6 steps of constants, 8 of addresses, 2 of pairs) and the 128 positions of a range;
    700 light states (six ranges of 128, 68 dummies)."""
    hmm = random_chain_hmm(700, S=20, seed=L, n_from_m=False)
    seqs = random_seqs(20, [L, L + 5, max(1, L - 3), L + 33, 2 * L + 1], seed=L)
    s, b, fb, _ = run(hmm, seqs)
    assert fb == 0
    oracle_check(hmm, seqs, s, b)


@pytest.mark.parametrize("L", [200, 256])
def test_diag2_wrap_lengths(sm2, L):
    """Two ranges (NP2 = 256 positions; 56 dummies or none): lengths around NP2 and 2 NP2, so that both
    diagonals of every lane cross position 0, and with it the ring's mirror end, once and twice and
    the row ends right before, at and after the crossing."""
    hmm = random_chain_hmm(L, S=5, seed=300 + L, n_from_m=False)
    lens = [255, 256, 257, 258, 511, 512, 513, 514, 193, 321]
    seqs = random_seqs(5, lens, seed=L)
    s, b, fb, plan = run(hmm, seqs)
    assert fb == 0
    oracle_check(hmm, seqs, s, b)


@pytest.mark.parametrize("S", [1, 2, 32])
def test_diag2_alphabets(sm2, S):
    """One symbol (a single pair of ring planes), two, and the 32-symbol maximum (ring 112 KB)."""
    hmm = random_chain_hmm(400, S=S, seed=40 + S, n_from_m=False)
    seqs = random_seqs(S, [250, 33, 96], seed=S)
    s, b, fb, _ = run(hmm, seqs)
    assert fb == 0
    oracle_check(hmm, seqs, s, b)


@pytest.mark.parametrize("variant", [dict(self_n=False), dict(c_from_m=False), dict(self_c=False),
                                     dict(gap=37), dict(zero_emis=0.2), dict(ties=True), dict(inf_edges=0.1),
                                     dict(start=(0, 5, 301)), dict(sx=True)])
def test_diag2_chain_variants(sm2, variant):
    """The chain-shaped edge cases of test_diag_chain_variants: no self loops, no sink term, chain
    breaks, +inf emissions and edges, exact ties, starts in light rows, S fed by N (the X_SF term)."""
    hmm = random_chain_hmm(600, S=12, seed=11, **variant)
    if variant.get("sx"):  # N -> C: the sink takes a term from the feeder row (PipeModel.sx)
        hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))
        hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(hmm.states_num - 1))
        hmm.trans_probs = np.append(hmm.trans_probs, np.float32(3.5))
        hmm.trans_num += 1
    seqs = random_seqs(12, [300, 64, 1, 97, 33], seed=12)
    s, b, _, _ = run(hmm, seqs)
    oracle_check(hmm, seqs, s, b)


def test_diag2_fallback_rows_match_oracle(sm2):
    """Models whose feeder row takes its light term (M -> N free): the check on the minimum of a
    lane's two scores fails, the combining wave's workgroup re-runs those rows in the same launch,
    every score matches the oracle; 1, 2 and 4 sequences per workgroup."""
    total_fb = 0
    for seed in range(8):
        hmm = random_chain_hmm(300 if seed < 6 else 700, S=8, seed=seed)
        rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
        probs = hmm.trans_probs.copy()
        probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
        hmm.trans_probs = probs
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        s, b, fb, _ = run(hmm, seqs)
        total_fb += fb
        oracle_check(hmm, seqs, s, b)
    assert total_fb > 0


@pytest.fixture(scope="module")
def chain_2405():
    """The chain kernel's scores of the first five headline rows, computed once."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))[:5]
    s, b, _, _ = run(hmm, seqs, kernel=CHAIN, want_sm=0)
    return hmm, seqs, s, b


@pytest.mark.parametrize("nseq", [1, 2, 3, 5])
def test_diag2_workgroup_widths(sm2, chain_2405, nseq):
    """1, 2 and 4 sequences per workgroup and a partial last group (3: one wave idle; 5: three) on
    2405.chmm (19 ranges of 128: the 64-wide count, 38, is even; 27 dummies), equal to the chain kernel."""
    hmm, seqs, sc, bc = chain_2405
    s, b, fb, plan = run(hmm, seqs[:nseq])
    assert plan["threads"] == 64 * (4 if nseq >= 4 else 2 if nseq >= 2 else 1), plan
    assert fb == 0
    assert_same(s, b, sc[:nseq], bc[:nseq])


def test_diag2_covid_ragged(sm2):
    """16 protein sequences of 38..7096 observations: ragged rows in one workgroup (waves whose row
    has ended keep refilling the shared ring)."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("covid-19.ess"))
    s, b, fb, _ = run(hmm, seqs)
    assert fb == 0
    sc, bc, _, _ = run(hmm, seqs, kernel=CHAIN, want_sm=0)
    assert_same(s, b, sc, bc)


@pytest.mark.parametrize("kern", [DIAG, _lib.SVH_KERNEL_AUTO])
def test_diag2_spec_tail_resumes_from_device_scores(sm2, kern):
    """_spec level 2 with the tail -- rows resumed at begin > 0 from the chunks' device scores (v_in) --
    forced onto the variant (the rule alone keeps resumed rows on one diagonal); tails of 0 and 1
    observations, a length-1 row; bit-exact against the oracle's level-2 association."""
    hmm = svh.read_HMM(chmm("100.chmm"))
    base = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    seqs = [base[0][:301], base[1][:64], base[2][:2], base[0][:1], base[1][:1000]]
    model = svh.DeviceModel(hmm, kernel=kern)
    model.spec_build(2)
    batch = model.batch(seqs)
    assert batch.plan(2)["diag_sm"] == 2, batch.plan(2)
    batch.run(2)
    s, _ = batch.read()
    batch.close()
    model.close()
    for q, seq in enumerate(seqs):
        ref = oracle.viterbi_spec(hmm, 2, seq)
        assert bit_equal(s[q], ref), (q, first_mismatch(s[q], ref))


def test_diag2_spec3_tail_equals_chain(sm2):
    """_spec level 3 (tails of 0, 1 and 2 observations) resumed on the variant against the serial
    chain kernel at level 3, bit-exact."""
    hmm = svh.read_HMM(chmm("1001.chmm"))
    base = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    seqs = [base[0][:258], base[1][:259], base[2][:260], base[0][:3]]
    out = []
    for kern in (DIAG, CHAIN):
        model = svh.DeviceModel(hmm, kernel=kern)
        model.spec_build(3)
        if kern == DIAG:
            batch = model.batch(seqs)
            assert batch.plan(3)["diag_sm"] == 2, batch.plan(3)
            batch.close()
        out.append(model.viterbi(seqs, level=3))
        model.close()
    assert_same(out[0][0], out[0][1], out[1][0], out[1][1])


def test_diag2_two_batches_two_streams(sm2):
    """Two batches in flight on two streams at once, each with its own scratch and partials."""
    import torch

    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))[:9]
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    model = svh.DeviceModel(hmm)
    a, b = model.batch(seqs), model.batch(seqs[::-1])
    assert a.plan()["kernel"] == DIAG and a.plan()["diag_sm"] == 2, a.plan()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        a.run(0, sa.cuda_stream)
        b.run(0, sb.cuda_stream)
        r1, k1 = a.read(sa.cuda_stream)
        r2, k2 = b.read(sb.cuda_stream)
        assert a.fallbacks() == 0 and b.fallbacks() == 0
        assert_same(r1, k1, r2[::-1], k2[::-1])
        for q in range(len(seqs)):
            assert hashlib.sha256(np.ascontiguousarray(r1[q]).tobytes()).hexdigest() == rows[q]["scores_sha256"], q
    a.close()
    b.close()
    model.close()


def test_diag2_headline_auto_goldens_digests_no_fallback(monkeypatch):
    """2405.chmm x emit_50_3500_20 through AUTO with no knob set: the variant the selection rule names
    (two diagonals where one per lane would stack waves on a SIMD: ceil(50 / 4) x 4 x 38 = 1,976 waves
    against 4 x CUs), the two golden rows bit-exact, every row against the committed digests, no row
    fell back."""
    monkeypatch.delenv("SVH_DIAG_SM", raising=False)
    g = load_golden("chmm2405_emit50")
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))
    model = svh.DeviceModel(hmm)
    info = model.info()
    batch = model.batch(seqs)
    plan = batch.plan()
    want = 2 if 52 * info["diag_ranges"] > 4 * info["cu_count"] else 1
    assert plan["kernel"] == DIAG and plan["threads"] == 256 and plan["diag_sm"] == want, plan
    few = model.batch(seqs[:13])  # 16 x 38 = 608 waves: one per SIMD already
    assert few.plan()["diag_sm"] == (2 if 16 * info["diag_ranges"] > 4 * info["cu_count"] else 1), few.plan()
    few.close()
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    batch.run()
    s, b = batch.read()
    assert batch.fallbacks() == 0
    for rec in g["sequences"]:
        q = rec["index"]
        assert bit_equal(s[q], from_hex(rec["scores"])), first_mismatch(s[q], from_hex(rec["scores"]))
        assert b[q] == rec["best_state"]
    for q in range(len(seqs)):
        assert hashlib.sha256(np.ascontiguousarray(s[q]).tobytes()).hexdigest() == rows[q]["scores_sha256"], q
        assert b[q] == rows[q]["best_state"], q
    batch.close()
    model.close()


def test_diag2_headline_forced_digests(sm2):
    """The 50 headline rows on the forced variant against the committed digests (whatever AUTO's
    rule chooses on the device at hand), no row fell back."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    s, b, fb, _ = run(hmm, seqs, kernel=_lib.SVH_KERNEL_AUTO)
    assert fb == 0
    for q in range(len(seqs)):
        assert hashlib.sha256(np.ascontiguousarray(s[q]).tobytes()).hexdigest() == rows[q]["scores_sha256"], q
        assert b[q] == rows[q]["best_state"], q


@pytest.mark.parametrize("name", ["100.chmm", "1001.chmm"])
def test_diag2_reference_models(sm2, name):
    """100.chmm (one range of 128, 30 dummies) and 1001.chmm (eight ranges; the 64-wide count is 16)
    x emit_3 under AUTO, forced onto the variant: equal to the chain kernel, one row against the
    oracle, no fallback."""
    hmm = svh.read_HMM(chmm(name))
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    s, b, fb, _ = run(hmm, seqs, kernel=_lib.SVH_KERNEL_AUTO)
    assert fb == 0
    oracle_check(hmm, seqs[:1], s[:1], b[:1])
    sc, bc, _, _ = run(hmm, seqs, kernel=CHAIN, want_sm=0)
    assert_same(s, b, sc, bc)
