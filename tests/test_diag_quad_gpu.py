"""GPU parity of the diagonal plan's quad ring (diag.hip, QD): two diagonals per lane with the loader
wave, every ring column one 16-byte entry {ea[c], ea[c + 64], eb[c], eb[c + 64]} read by one LDS
instruction per step, the ring [S][5 x 64 + 64 mirror] quads refilled by the loader wave with one
LDS-DMA instruction per symbol and group from PipeModel::dtab4.

Every test forces SVH_DIAG_SM=2, SVH_DIAG_LOADER=1 and SVH_DIAG_QUAD=1 (read when the model is
created), asserts that the batch's plan says DIAG, two diagonals and `diag_quad` (svh_batch_diag_quad,
which `plan()` adds to svh_batch_plan's fields), and compares scores and
best states bit-exact with the oracle and with the same batch under SVH_DIAG_QUAD=0 (the plane layout),
with equal fallback counts.  The shapes: lengths across one to six blocks of 64 steps with rows of
different lengths in one workgroup; position spaces of 128 and 256 positions that wrap onto themselves
((c + 64) % NP folding onto the same range, the mirror crossed more than twice); alphabets of 1, 2 and 20
symbols, the largest whose quad ring fits the CU's LDS and the first that does not (the plan then says
plane layout although forced); 1, 2 and 4 step waves with idle waves; rows whose speculation fails (the
re-run after the loader wave has ended); two batches in flight on two streams; the reference models
under AUTO.
"""
import hashlib

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.conftest import chmm, ess
from tests.helpers import bit_equal, first_mismatch, load_digests, random_chain_hmm, random_seqs

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def quad_lds_bytes(waves, S, sx=False):
    """diag.hip diag_lds_main(W, S, sx, 2, true, true): the quad ring [S][384] float4, the symbol
    template [S][8], three stream buffers of 64 steps per wave (constants 4 floats, ring address 1,
    X_SF 1 where the model has it), two words per wave."""
    return (S * 384 * 4 + S * 8 + waves * 3 * 64 * (5 + (1 if sx else 0)) + 2 * waves) * 4


def forced(monkeypatch, quad):
    monkeypatch.setenv("SVH_DIAG_SM", "2")
    monkeypatch.setenv("SVH_DIAG_LOADER", "1")
    monkeypatch.setenv("SVH_DIAG_QUAD", "1" if quad else "0")


def run(monkeypatch, hmm, seqs, quad, kernel=DIAG, want_quad=None):
    forced(monkeypatch, quad)
    model = svh.DeviceModel(hmm, kernel=kernel)
    b = model.batch(seqs)
    plan = b.plan()
    want = (1 if quad else 0) if want_quad is None else want_quad
    assert plan["kernel"] == DIAG and plan["diag_sm"] == 2 and plan["diag_quad"] == want, plan
    if want:
        waves = 4 if len(seqs) >= 4 else 2 if len(seqs) >= 2 else 1
        assert plan["diag_quad_lds_bytes"] == quad_lds_bytes(waves, hmm.emit_num, sx=True), plan  # (reported with the X_SF stream)
    else:
        assert plan["diag_quad_lds_bytes"] == 0, plan
    b.run()
    s, best = b.read()
    fb = b.fallbacks()
    b.close()
    model.close()
    return s, best, fb


def assert_same(s1, b1, s2, b2):
    for q in range(len(s1)):
        assert bit_equal(s1[q], s2[q]), (q, first_mismatch(s1[q], s2[q]))
    assert np.array_equal(b1, b2)


def oracle_check(hmm, seqs, scores, best):
    refs = oracle.viterbi_batch(hmm, seqs)[0]
    for q in range(len(seqs)):
        assert bit_equal(scores[q], refs[q]), (q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (q, best[q], ref_best)


def three_ways(monkeypatch, hmm, seqs, kernel=DIAG, want_quad=1):
    """The quad ring against the oracle and against the plane layout; its fallback rows."""
    s, b, fb = run(monkeypatch, hmm, seqs, True, kernel, want_quad)
    oracle_check(hmm, seqs, s, b)
    s0, b0, fb0 = run(monkeypatch, hmm, seqs, False, kernel)
    assert_same(s, b, s0, b0)
    assert fb == fb0
    return fb


@pytest.mark.parametrize("L", [1, 2, 59, 64, 65, 66, 123, 128, 129, 130, 187, 192, 193, 194, 257, 385])
def test_quad_sequence_lengths(monkeypatch, L):
    """One to six blocks: rows that end right before, at and after a block's end, at the prefetch
    distances behind it and past the ring's five groups; five rows of different lengths per workgroup
    (one of four step waves, one of a single real wave).  700 light states (NP = 768), S = 20."""
    hmm = random_chain_hmm(700, S=20, seed=L, n_from_m=False)
    seqs = random_seqs(20, [L, 1, L + 64, 3 * L + 1, max(1, L - 3)], seed=L)
    assert three_ways(monkeypatch, hmm, seqs) == 0


@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 200, 256])
def test_quad_wrap(monkeypatch, L):
    """Position spaces of one range (NP = 128: the quad's second column, c + 64, folds onto the same
    range) and of two (NP = 256), full and with +inf dummies; rows longer than twice NP, so that every
    lane crosses position 0 and the ring's mirror more than twice."""
    hmm = random_chain_hmm(L, S=6, seed=100 + L, n_from_m=False)
    seqs = random_seqs(6, [3 * (L + 2) + 5, 700, 64], seed=L)
    assert max(len(s) for s in seqs) > 2 * 128 * ((L + 127) // 128)
    assert three_ways(monkeypatch, hmm, seqs) == 0


def fit_bounds(waves):
    """The largest alphabet whose quad launch of that many step waves fits, and the first that does not."""
    fit = max(S for S in range(1, 33) if quad_lds_bytes(waves, S) <= LDS_MAX)
    assert 20 < fit < 32, fit
    return fit, fit + 1


@pytest.mark.parametrize("which", ["1", "2", "20", "largest"])
def test_quad_alphabets(monkeypatch, which):
    """S LDS-DMA instructions per group: one symbol, two, the headline's 20 and the largest alphabet
    whose ring fits beside two step waves' streams (the last DMA ends below the LDS the launch asks for)."""
    S = fit_bounds(2)[0] if which == "largest" else int(which)
    hmm = random_chain_hmm(400, S=S, seed=40 + S, n_from_m=False)
    seqs = random_seqs(S, [250, 33, 96], seed=S)
    assert quad_lds_bytes(2, S) <= LDS_MAX
    assert three_ways(monkeypatch, hmm, seqs) == 0


def test_quad_first_alphabet_that_does_not_fit(monkeypatch):
    """One symbol more than fits: the plan says plane layout although the quad ring is forced, and the
    results are exact."""
    S = fit_bounds(2)[1]
    hmm = random_chain_hmm(400, S=S, seed=40 + S, n_from_m=False)
    seqs = random_seqs(S, [250, 33, 96], seed=S)
    assert quad_lds_bytes(2, S) > LDS_MAX
    assert three_ways(monkeypatch, hmm, seqs, want_quad=0) == 0


@pytest.mark.parametrize("nseq", [1, 2, 3, 5])
def test_quad_workgroup_widths(monkeypatch, nseq):
    """1, 2 and 4 step waves beside the loader wave (the prologue's fill spread over them), and partial
    last groups (3: one wave idle; 5: three)."""
    hmm = random_chain_hmm(700, S=20, seed=77, n_from_m=False)
    seqs = random_seqs(20, [333, 200, 64, 401, 130][:nseq], seed=78)
    forced(monkeypatch, True)
    model = svh.DeviceModel(hmm, kernel=DIAG)
    batch = model.batch(seqs)
    assert batch.plan()["threads"] == 64 * (4 if nseq >= 4 else 2 if nseq >= 2 else 1), batch.plan()
    batch.close()
    model.close()
    assert three_ways(monkeypatch, hmm, seqs) == 0


def test_quad_fallback_rows_match_oracle(monkeypatch):
    """Models whose feeder row takes its light term (M -> N free): the speculation fails and the step
    waves re-run those rows exactly, in the same launch, after the loader wave has ended (the re-run's
    scores overwrite the ring); 1, 2 and 4 sequences per workgroup."""
    total_fb = 0
    for seed in range(6):
        hmm = random_chain_hmm(300 if seed < 4 else 700, S=8, seed=seed)
        rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
        probs = hmm.trans_probs.copy()
        probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
        hmm.trans_probs = probs
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        total_fb += three_ways(monkeypatch, hmm, seqs)
    assert total_fb > 0


def test_quad_two_batches_two_streams(monkeypatch):
    """Two batches in flight on two streams at once, each with its own scratch and partials: nine
    headline rows, three times, against the committed digests."""
    import torch

    forced(monkeypatch, True)
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))[:9]
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    model = svh.DeviceModel(hmm)
    a, b = model.batch(seqs), model.batch(seqs[::-1])
    for x in (a, b):
        assert x.plan()["kernel"] == DIAG and x.plan()["diag_sm"] == 2 and x.plan()["diag_quad"] == 1, x.plan()
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
            assert k1[q] == rows[q]["best_state"], q
    a.close()
    b.close()
    model.close()


@pytest.mark.parametrize("name", ["100.chmm", "1001.chmm"])
def test_quad_reference_models(monkeypatch, name):
    """100.chmm and 1001.chmm x emit_3 under AUTO with the variant forced: no row fell back, bit-exact
    with the oracle and with the plane layout."""
    hmm = svh.read_HMM(chmm(name))
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    assert three_ways(monkeypatch, hmm, seqs, kernel=_lib.SVH_KERNEL_AUTO) == 0
