"""GPU parity of decoded paths on the diagonal plan (diag.hip PATHS + the diagonal traceback of
pipe_paths.hip), the route of path batches of models created with kernel=SVH_KERNEL_DIAG.

The forward kernel records a decision bit per light cell (diagonal-major words), light-score
checkpoints every 32 observations, F and sink checkpoints every 32 and the ranges' light minima of
every observation (folded every 8 steps); the walk rebuilds the sink's score between checkpoints.
Every case checks scores (bit for bit), best states and every path entry against the oracle's
decode or the committed digests.  Rows whose speculation fails go to the chain kernel's path
variant, which would also hide a wrong record: reference workloads assert that no row fell back.
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
TODAY = (_lib.SVH_KERNEL_CHAIN, _lib.SVH_KERNEL_FUSED, _lib.SVH_KERNEL_GENERIC)  # a declined model's route


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def decode_check(hmm, seqs, expect=(DIAG,)):
    """One decoded-path batch of a SVH_KERNEL_DIAG model against the oracle's decode; returns the
    rows that fell back and the batch's plan."""
    model = svh.DeviceModel(hmm, kernel=DIAG)
    batch = model.batch(seqs, paths=True)
    plan = batch.plan()
    assert plan["kernel"] in expect, plan
    batch.run()
    s, b, pth = batch.read(want_paths=True)
    fb = batch.fallbacks()
    for q, seq in enumerate(seqs):
        ref, ref_best, ref_path = oracle.decode(hmm, seq)
        assert bit_equal(s[q], ref), (q, first_mismatch(s[q], ref))
        assert b[q] == ref_best, (q, b[q], ref_best)
        assert np.array_equal(pth[q], ref_path), (q, np.nonzero(pth[q] != ref_path)[0][:5], len(seq))
    batch.close()
    model.close()
    return fb, plan


def sha(a, dtype=None):
    return hashlib.sha256(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)).tobytes()).hexdigest()


def digest_check(rows, s, b, pth, order=None):
    for q in range(len(rows)):
        r = rows[q if order is None else order[q]]
        assert sha(s[q]) == r["scores_sha256"], q
        assert b[q] == r["best_state"], q
        assert sha(pth[q], np.int32) == r["path_sha256"], q


def test_diag_paths_plan():
    """A SVH_KERNEL_DIAG model of 2405.chmm reports the diagonal plan as its path kernel, a
    3-sequence path batch plans two waves on it, and scores-only batches of the same model keep
    the diagonal plan and their digests after a path batch has run."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))[:3]
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    model = svh.DeviceModel(hmm, kernel=DIAG)
    assert model.info()["paths_kernel"] == DIAG
    pb = model.batch(seqs, paths=True)
    plan = pb.plan()
    assert plan["kernel"] == DIAG and plan["threads"] == 128 and plan["slots"] == 1, plan
    assert 0 < plan["lds_bytes"] <= 80 * 1024, plan
    sb = model.batch(seqs)
    assert sb.plan()["kernel"] == DIAG
    sb.run()
    s0, b0 = sb.read()
    pb.run()
    s, b, pth = pb.read(want_paths=True)
    assert pb.fallbacks() == 0
    digest_check(rows[:3], s, b, pth)
    sb.run()
    s1, b1 = sb.read()
    for q in range(3):
        assert sha(s0[q]) == rows[q]["scores_sha256"] and sha(s1[q]) == rows[q]["scores_sha256"], q
    assert np.array_equal(b0, b1)
    pb.close()
    sb.close()
    model.close()


@pytest.mark.parametrize("L", [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 97, 127, 128, 129, 321, 1025])
def test_diag_paths_sequence_lengths(L):
    """The fold (every 8 steps), the mask word, the checkpoints and the sink checkpoint (every 32),
    the 64-step block, the tail block and one full turn of the 320-column ring."""
    hmm = random_chain_hmm(700, S=20, seed=L, n_from_m=False)
    fb, _ = decode_check(hmm, random_seqs(20, [L, L + 5, max(1, L - 3)], seed=L))
    assert fb == 0  # (no M -> N term: the check cannot fail, the diagonal records made every path)


@pytest.mark.parametrize("L", [1, 62, 64, 128, 129])
def test_diag_paths_diagonal_wrap(L):
    """Few light rows, long sequences: the diagonal index (p - t) mod NP wraps many times, with
    NP == light rows (64, 128) and with dummy positions."""
    hmm = random_chain_hmm(L, S=6, seed=100 + L, n_from_m=False)
    fb, _ = decode_check(hmm, random_seqs(6, [3 * (L + 2) + 5, 700, 64], seed=L))
    assert fb == 0


@pytest.mark.parametrize("nseq", [1, 2, 3, 5])
def test_diag_paths_workgroup_widths(nseq):
    """One, two and four sequences per workgroup, idle waves, a finished wave beside a running one."""
    hmm = random_chain_hmm(300, S=20, seed=7, n_from_m=False)
    fb, _ = decode_check(hmm, random_seqs(20, [700, 1, 40, 333, 64][:nseq], seed=nseq))
    assert fb == 0


VARIANTS = [dict(), dict(self_n=False), dict(c_from_m=False), dict(self_c=False), dict(gap=37), dict(zero_emis=0.2),
            dict(ties=True), dict(inf_edges=0.1), dict(start=(0, 5, 301)), dict(n_from_m=False)]


@pytest.mark.parametrize("variant", VARIANTS)
def test_diag_paths_chain_variants(variant):
    """MSV-shaped random models (ties, chain breaks, +inf edges, starts in light rows, no self
    loops): every path entry equal to the oracle's decode.  (With M -> N terms a row's check may
    fail and the chain fallback decode it: the next test pins the diagonal records.)"""
    hmm = random_chain_hmm(600, S=12, seed=11, **variant)
    decode_check(hmm, random_seqs(12, [300, 64, 1, 97, 700], seed=12))


@pytest.mark.parametrize("variant", [v for v in VARIANTS if "n_from_m" not in v and "self_n" not in v])
def test_diag_paths_chain_variants_no_fallback(variant):
    """The same variants without the M -> N terms: the check cannot fail, so no row may fall back
    and every path comes from the diagonal records.  (Not self_n=False: with neither term N would
    have no row at all, which is no chain model.)"""
    hmm = random_chain_hmm(600, S=12, seed=11, **dict(variant, n_from_m=False))
    fb, _ = decode_check(hmm, random_seqs(12, [300, 64, 1, 97, 700], seed=12))
    assert fb == 0


@pytest.mark.parametrize("nseq", [1, 2, 5])
def test_diag_paths_sink_fed_by_feeder_declined(nseq):
    """N -> C: the sink takes a term from the feeder row (PipeModel.sx).  The path variant has no
    such instantiation: the model keeps today's route at every batch width, plan() says so, and the
    results are the oracle's."""
    hmm = random_chain_hmm(600, S=12, seed=11)
    hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))
    hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(hmm.states_num - 1))
    hmm.trans_probs = np.append(hmm.trans_probs, np.float32(3.5))
    hmm.trans_num += 1
    model = svh.DeviceModel(hmm, kernel=DIAG)
    assert model.info()["paths_kernel"] in TODAY
    model.close()
    _, plan = decode_check(hmm, random_seqs(12, [300, 64, 1, 97, 700][:nseq], seed=12), expect=TODAY)
    assert plan["kernel"] in TODAY, plan


def test_diag_paths_heavy_run_and_jstar():
    """covid-19 sequences whose best paths run N -> match states -> C on 2405.chmm: the heavy-run
    walk over the rebuilt sink scores and the j* recompute at the entry into C."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("covid-19.ess"))
    short = [s for s in seqs if len(s) < 1500][:4]
    fb, _ = decode_check(hmm, short)
    assert fb == 0


def test_diag_paths_fallback_rows_match_oracle():
    """Models whose feeder row takes its light term: those rows run on the chain kernel's path
    variant and its traceback, the others on the diagonal plan; every path equals the oracle's."""
    total_fb = 0
    for seed in range(6):
        hmm = random_chain_hmm(300, S=8, seed=seed)
        rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
        probs = hmm.trans_probs.copy()
        probs[(cols == 0) & (rows != 0)] = np.float32(0.0)
        hmm.trans_probs = probs
        fb, _ = decode_check(hmm, random_seqs(8, [700, 1, 40, 333], seed=seed))
        total_fb += fb
    assert total_fb > 0


def test_diag_paths_declined_no_feeder_term():
    """One N -> M_j transition deleted: F does not win every tie (ties_heavy is false), the model
    keeps today's route and its results."""
    hmm = random_chain_hmm(300, S=8, seed=3, n_from_m=False)
    keep = ~((hmm.trans_rows == 0) & (hmm.trans_cols == 150))
    assert keep.sum() == hmm.trans_num - 1
    hmm.trans_rows, hmm.trans_cols, hmm.trans_probs = hmm.trans_rows[keep], hmm.trans_cols[keep], hmm.trans_probs[keep]
    hmm.trans_num -= 1
    _, plan = decode_check(hmm, random_seqs(8, [333, 64, 1], seed=3), expect=(DIAG,) + TODAY)
    assert plan["kernel"] in TODAY, plan


def test_diag_paths_declined_or_planned_32_symbols():
    """32 symbols: the table ring alone is past the variant's LDS bound; whichever route the plan
    reports, the results are the oracle's."""
    hmm = random_chain_hmm(400, S=32, seed=72, n_from_m=False)
    decode_check(hmm, random_seqs(32, [250, 33, 96], seed=32), expect=(DIAG,) + TODAY)


@pytest.mark.parametrize("name", ["100.chmm", "1001.chmm", "2405.chmm"])
def test_diag_paths_reference_models_vs_oracle(name):
    hmm = svh.read_HMM(chmm(name))
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))[:3]
    fb, _ = decode_check(hmm, seqs)
    assert fb == 0


@pytest.mark.parametrize("ess_name", ["emit_50_3500_20.ess", "covid-19.ess"])
def test_diag_paths_headline_digests(ess_name):
    """2405.chmm x emit_50_3500_20 (all 50 rows) and x covid-19 (all 16 ragged rows): scores, best
    states and paths against the committed oracle digests, run twice on one batch, no fallback row."""
    rows = load_digests()[f"2405.chmm x {ess_name}"]
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess(ess_name))
    model = svh.DeviceModel(hmm, kernel=DIAG)
    batch = model.batch(seqs, paths=True)
    assert batch.plan()["kernel"] == DIAG
    for _ in range(2):
        batch.run()
        s, b, pth = batch.read(want_paths=True)
        assert batch.fallbacks() == 0
        digest_check(rows, s, b, pth)
    batch.close()
    model.close()


def test_diag_paths_two_batches_two_streams():
    """Two path batches in flight on two streams at once, the headline and its reverse, three
    rounds: each batch owns its records."""
    import torch

    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess"]
    rev = list(range(len(seqs)))[::-1]
    model = svh.DeviceModel(hmm, kernel=DIAG)
    a, b = model.batch(seqs, paths=True), model.batch(seqs[::-1], paths=True)
    assert a.plan()["kernel"] == DIAG and b.plan()["kernel"] == DIAG
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        a.run(0, sa.cuda_stream)
        b.run(0, sb.cuda_stream)
        s1, k1, p1 = a.read(sa.cuda_stream, want_paths=True)
        s2, k2, p2 = b.read(sb.cuda_stream, want_paths=True)
        assert a.fallbacks() == 0 and b.fallbacks() == 0
        digest_check(rows, s1, k1, p1)
        digest_check(rows, s2, k2, p2, order=rev)
    a.close()
    b.close()
    model.close()
