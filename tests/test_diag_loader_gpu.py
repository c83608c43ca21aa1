"""GPU parity of the diagonal plan's loader-wave variant (diag.hip, LD): the workgroup runs one wave
more than it has sequences; that wave refills the shared ring and builds the three streams of every
sequence two blocks ahead (three stream buffers), the step waves only step and meet it at one barrier
per block, and it ends before the epilogue (the combine and the exact re-run see the step waves only).

Every test forces the variant (SVH_DIAG_LOADER=1, read when the model is created) with one or two
diagonals per lane (SVH_DIAG_SM), asserts that the batch's plan says DIAG with that many diagonals, and
compares scores and best states bit-exact with the oracle and with the same batch under
SVH_DIAG_LOADER=0.  The shapes: lengths across one to six blocks of 64 steps (the period of the three
buffers twice over) with rows of different lengths in one workgroup, so that per-wave block counts
differ from the workgroup's; 1, 2 and 4 step waves and groups with idle waves; alphabets whose 32 S
refill chunks are half a pass, one pass and 16 passes of the loader's 64 lanes; position spaces that
wrap onto themselves; rows whose speculation fails (the re-run after the loader wave has gone); two
batches in flight at once.
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


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def run(monkeypatch, hmm, seqs, loader, sm, kernel=DIAG):
    monkeypatch.setenv("SVH_DIAG_LOADER", "1" if loader else "0")
    monkeypatch.setenv("SVH_DIAG_SM", str(sm))
    model = svh.DeviceModel(hmm, kernel=kernel)
    b = model.batch(seqs)
    plan = b.plan()
    assert plan["kernel"] == DIAG and plan["diag_sm"] == sm, plan
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


_refs = {}


def oracle_check(key, hmm, seqs, scores, best):
    """Against the oracle's rows of this case, computed once for both diagonal counts."""
    if key not in _refs:
        _refs[key] = oracle.viterbi_batch(hmm, seqs)[0]
    refs = _refs[key]
    for q in range(len(seqs)):
        assert bit_equal(scores[q], refs[q]), (q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (q, best[q], ref_best)


def both(monkeypatch, key, hmm, seqs, sm, kernel=DIAG):
    """The loader-wave variant against the oracle and against the plain variant; its fallback rows."""
    s, b, fb = run(monkeypatch, hmm, seqs, True, sm, kernel)
    oracle_check(key, hmm, seqs, s, b)
    s0, b0, fb0 = run(monkeypatch, hmm, seqs, False, sm, kernel)
    assert_same(s, b, s0, b0)
    assert fb == fb0
    return fb


@pytest.mark.parametrize("sm", [1, 2])
@pytest.mark.parametrize("L", [1, 2, 59, 64, 65, 66, 123, 128, 129, 130, 187, 192, 193, 194, 257, 385])
def test_loader_sequence_lengths(monkeypatch, sm, L):
    """One to six blocks and the three-buffer period: rows that end right before, at and after a block's
    end, at the prefetch distances behind it (constants 6, ring addresses 8 steps ahead: 59, 123, 187
    observations are 58, 122, 186 steps) and past twice the period; five rows of different lengths in
    one workgroup of four step waves and one of a single real wave.  700 light states, S = 20."""
    hmm = random_chain_hmm(700, S=20, seed=L, n_from_m=False)
    seqs = random_seqs(20, [L, 1, L + 64, 3 * L + 1, max(1, L - 3)], seed=L)
    assert both(monkeypatch, ("len", L), hmm, seqs, sm) == 0


@pytest.mark.parametrize("sm", [1, 2])
@pytest.mark.parametrize("nseq", [1, 2, 3, 5])
def test_loader_workgroup_widths(monkeypatch, sm, nseq):
    """1, 2 and 4 step waves beside the loader wave, and partial last groups (3: one wave idle; 5: three)."""
    hmm = random_chain_hmm(700, S=20, seed=77, n_from_m=False)
    seqs = random_seqs(20, [333, 200, 64, 401, 130][:nseq], seed=78)
    monkeypatch.setenv("SVH_DIAG_LOADER", "1")
    monkeypatch.setenv("SVH_DIAG_SM", str(sm))
    model = svh.DeviceModel(hmm, kernel=DIAG)
    batch = model.batch(seqs)
    assert batch.plan()["threads"] == 64 * (4 if nseq >= 4 else 2 if nseq >= 2 else 1), batch.plan()
    batch.close()
    model.close()
    assert both(monkeypatch, ("width", nseq), hmm, seqs, sm) == 0


@pytest.mark.parametrize("sm", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 32])
def test_loader_alphabets(monkeypatch, sm, S):
    """32 S refill chunks over the loader's 64 lanes: half a pass (the clamp), one pass, all 16."""
    hmm = random_chain_hmm(400, S=S, seed=40 + S, n_from_m=False)
    seqs = random_seqs(S, [250, 33, 96], seed=S)
    assert both(monkeypatch, ("alpha", S), hmm, seqs, sm) == 0


@pytest.mark.parametrize("sm", [1, 2])
@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 200, 256])
def test_loader_wrap(monkeypatch, sm, L):
    """Position spaces of one and two ranges (of 64 or of 128 diagonals), full and with dummies; rows
    longer than twice the position space, so that every lane crosses position 0 and the ring's
    mirror more than twice."""
    hmm = random_chain_hmm(L, S=6, seed=100 + L, n_from_m=False)
    seqs = random_seqs(6, [3 * (L + 2) + 5, 700, 64], seed=L)
    assert both(monkeypatch, ("wrap", L), hmm, seqs, sm) == 0


@pytest.mark.parametrize("sm", [1, 2])
def test_loader_fallback_rows_match_oracle(monkeypatch, sm):
    """Models whose feeder row takes its light term (M -> N free): the speculation fails and the step
    waves re-run those rows exactly, in the same launch, after the loader wave has ended; 1, 2 and 4
    sequences per workgroup."""
    total_fb = 0
    for seed in range(6):
        hmm = random_chain_hmm(300 if seed < 4 else 700, S=8, seed=seed)
        rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
        probs = hmm.trans_probs.copy()
        probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
        hmm.trans_probs = probs
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        total_fb += both(monkeypatch, ("fallback", seed), hmm, seqs, sm)
    assert total_fb > 0


@pytest.mark.parametrize("sm", [1, 2])
def test_loader_two_batches_two_streams(monkeypatch, sm):
    """Two batches in flight on two streams at once, each with its own scratch and partials."""
    import torch

    monkeypatch.setenv("SVH_DIAG_LOADER", "1")
    monkeypatch.setenv("SVH_DIAG_SM", str(sm))
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))[:9]
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    model = svh.DeviceModel(hmm)
    a, b = model.batch(seqs), model.batch(seqs[::-1])
    assert a.plan()["kernel"] == DIAG and a.plan()["diag_sm"] == sm, a.plan()
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


@pytest.mark.parametrize("sm", [1, 2])
@pytest.mark.parametrize("name", ["100.chmm", "1001.chmm"])
def test_loader_reference_models(monkeypatch, sm, name):
    """100.chmm and 1001.chmm x emit_3 under AUTO with the variant forced: no row fell back, bit-exact
    with the oracle and with the plain variant."""
    hmm = svh.read_HMM(chmm(name))
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    assert both(monkeypatch, ("ref", name), hmm, seqs, sm, kernel=_lib.SVH_KERNEL_AUTO) == 0


@pytest.mark.parametrize("sm", [1, 2])
def test_loader_step_floor_leaves_results(monkeypatch, sm):
    """svh_batch_step_floor_ms on a diagonal-plan batch (the loader-wave launch with the loader wave
    idle, no LDS reads in the steps and no combine or re-run, scores into a scratch buffer): a
    positive time, and the batch's
    scores, best states and fallback count are what they were, for rows that pass the speculation
    check and for rows that fail it (no re-run may start from the floor launch's wrong scores)."""
    monkeypatch.setenv("SVH_DIAG_SM", str(sm))
    monkeypatch.delenv("SVH_DIAG_LOADER", raising=False)
    for free_feeder in (False, True):
        hmm = random_chain_hmm(300, S=8, seed=2)
        if free_feeder:  # M -> N free: the feeder row takes its light term
            rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
            probs = hmm.trans_probs.copy()
            probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
            hmm.trans_probs = probs
        seqs = random_seqs(8, [700, 1, 40, 333, 64], seed=2)
        model = svh.DeviceModel(hmm, kernel=DIAG)
        batch = model.batch(seqs)
        assert batch.plan()["kernel"] == DIAG and batch.plan()["diag_sm"] == sm, batch.plan()
        batch.run()
        s1, b1 = batch.read()
        fb1 = batch.fallbacks()
        assert batch.step_floor_ms(3) > 0
        s2, b2 = batch.read()
        assert_same(s1, b1, s2, b2)
        assert batch.fallbacks() == fb1
        batch.run()
        s3, b3 = batch.read()
        oracle_check(("floor", free_feeder), hmm, seqs, s3, b3)
        batch.close()
        model.close()
