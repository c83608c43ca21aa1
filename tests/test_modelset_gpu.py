"""GPU parity of model sets (svh_batchset_*, DeviceModelSet / DeviceBatchSet): one batch of sequences
scored against many models, the members on the diagonal plan in ONE launch of diag_set_kernel
(diag.hip), each workgroup finding its member from its block index.

Every case compares every member bit for bit with the oracle and with the same model's stand-alone
DeviceBatch run (scores and best states), and asserts how many members the set launch took
(`grouped`) and how many launches the run made.  A row whose speculation fails is re-run exactly in
the same launch, which would also hide a wrong grouped row: reference workloads assert that no row
fell back, and the re-run case asserts which member's rows did.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.conftest import DATA, chmm, ess
from tests.helpers import GOLDEN, bit_equal, first_mismatch, random_chain_hmm, random_hmm, random_seqs

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def waves_for(nseq):
    return 4 if nseq >= 4 else 2 if nseq >= 2 else 1


def set_lds(W, S):
    """The scores variant's LDS without an X_SF stream (diag.hip diag_lds_main): ring [S][320 + 64]
    float2, symbol template [S][8], constants and ring addresses [W][2][64] x 5 floats, 2 W words;
    larger than the re-run's 2 P + 2 W floats for the models of these tests."""
    return (S * 384 * 2 + S * 8 + W * 2 * 64 * 5 + 2 * W) * 4


def free_feeder(hmm, weight):
    """M_j -> N at `weight` for every j (0: N takes its light term, the speculation fails; +inf: never)."""
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    probs = hmm.trans_probs.copy()
    probs[(cols == 0) & (rows != 0)] = np.float32(weight)
    hmm.trans_probs = probs
    return hmm


def check_member(tag, hmm, seqs, scores, best, model=None):
    """Row by row against the oracle, and against the model's stand-alone batch."""
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    for q in range(len(seqs)):
        assert bit_equal(scores[q], refs[q]), (tag, q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, (tag, q, best[q], ref_best)
    if model is not None:
        b = model.batch(seqs)
        b.run()
        s1, b1 = b.read()
        b.close()
        for q in range(len(seqs)):
            assert bit_equal(scores[q], s1[q]), (tag, "stand-alone", q, first_mismatch(scores[q], s1[q]))
        assert np.array_equal(best, b1), (tag, "stand-alone best")


def run_set(hmms, seqs, kernels=None, level=0, first=()):
    """Create the models and the set, run once, check every member (the members in `first` first);
    returns (info, [fallbacks per member], [plan per member])."""
    kernels = kernels or [_lib.SVH_KERNEL_AUTO] * len(hmms)
    models = [svh.DeviceModel(h, kernel=k) for h, k in zip(hmms, kernels)]
    bs = svh.DeviceModelSet(models).batch(seqs)
    assert bs.info()["launches"] == 0
    bs.run(level)
    res = bs.read()
    info = bs.info()
    order = list(first) + [i for i in range(len(hmms)) if i not in first]
    for i in order:
        check_member(i, hmms[i], seqs, res[i][0], res[i][1], models[i])
    fbs = [b.fallbacks() for b in bs.members]
    plans = [b.plan() for b in bs.members]
    bs.close()
    for m in models:
        m.close()
    return info, fbs, plans


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("nseq", [1, 2, 3, 4, 5])
def test_set_entry_lookup_edges(nseq, rev):
    """Members of 1, 1, 1, 2 and 3 ranges (1, 63, 64, 65, 129 light rows), in that order and reversed:
    every first[] boundary has a one-block neighbour.  1 .. 5 sequences: one, two and four per
    workgroup and a last group with padded waves; lengths at the blocks' edges."""
    L = [1, 63, 64, 65, 129]
    hmms = [random_chain_hmm(l, S=20, seed=10 + l, n_from_m=False) for l in (L[::-1] if rev else L)]
    lens = [1, 2, 64, 65, 130]
    seqs = random_seqs(20, [lens[(q + nseq) % 5] for q in range(nseq)], seed=nseq)
    info, fbs, plans = run_set(hmms, seqs)
    W = waves_for(nseq)
    assert info["members"] == 5 and info["grouped"] == 5 and info["launches"] == 1, info
    assert info["waves"] == W and info["grid"] == -(-nseq // W) * (1 + 1 + 1 + 2 + 3), info
    assert all(p["kernel"] == DIAG for p in plans) and fbs == [0] * 5, (plans, fbs)


def test_set_more_than_64_entries():
    """70 members of 3 .. 72 light rows, one sequence of 70 observations: the lookup's second chunk of
    64 entries; members 0, 63, 64 and 69 are checked first."""
    hmms = [random_chain_hmm(3 + i, S=6, seed=200 + i, n_from_m=False) for i in range(70)]
    seqs = random_seqs(6, [70], seed=7)
    info, fbs, _ = run_set(hmms, seqs, first=(0, 63, 64, 69))
    assert info["grouped"] == 70 and info["launches"] == 1 and info["waves"] == 1, info
    assert info["grid"] == sum(-(-(3 + i) // 64) for i in range(70)), info
    assert fbs == [0] * 70


def test_set_alphabets_and_lds():
    """Members of 3, 20 and 32 symbols (sequences over the first 3): each workgroup lays its LDS out
    for its own alphabet; the launch asks for the largest member's footprint."""
    hmms = [random_chain_hmm(100, S=S, seed=300 + S, n_from_m=False) for S in (3, 20, 32)]
    seqs = random_seqs(3, [200, 65], seed=8)
    info, fbs, _ = run_set(hmms, seqs)
    assert info["grouped"] == 3 and info["launches"] == 1 and info["waves"] == 2, info
    assert info["lds_bytes"] == set_lds(2, 32), (info, set_lds(2, 32))
    assert fbs == [0] * 3


def test_set_rerun_sees_its_own_member():
    """A member whose feeder row takes its light term (M -> N free, the construction of
    test_pipe_gpu.py's fallback test) between two whose M -> N weight is +inf: the in-launch re-run
    (pipe_rerun_row) must run with the middle member's model and batch.  Only the middle member
    reports re-run rows, over the seeds at least one, and all three are exact."""
    middle = 0
    for seed in range(8):
        n = 300 if seed < 6 else 700
        hmms = [free_feeder(random_chain_hmm(n - 37, S=8, seed=50 + seed), np.inf),
                free_feeder(random_chain_hmm(n, S=8, seed=seed), 0.0),
                free_feeder(random_chain_hmm(n + 70, S=8, seed=90 + seed), np.inf)]
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        info, fbs, _ = run_set(hmms, seqs, kernels=[DIAG] * 3)
        assert info["grouped"] == 3 and info["launches"] == 1, info
        assert fbs[0] == 0 and fbs[2] == 0, (seed, fbs)
        middle += fbs[1]
    assert middle > 0


def test_set_mixed_eligibility():
    """A general model, a chain model whose light rows take a term from C as well (no pipelined plan)
    and a model created with SVH_KERNEL_CHAIN beside two grouped ones: two members in the set launch,
    three runs of their own after it, every member exact."""
    hmms = [random_chain_hmm(150, S=12, seed=401, n_from_m=False), random_hmm(200, S=12, seed=402),
            random_chain_hmm(130, S=12, seed=403, feed_c=True), random_chain_hmm(140, S=12, seed=404, n_from_m=False),
            random_chain_hmm(70, S=12, seed=405, n_from_m=False)]
    kernels = [_lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_CHAIN, DIAG]
    seqs = random_seqs(12, [130, 64, 3], seed=9)
    info, fbs, plans = run_set(hmms, seqs, kernels=kernels)
    assert info["members"] == 5 and info["grouped"] == 2 and info["launches"] == 1 + 3, info
    assert plans[0]["kernel"] == DIAG and plans[4]["kernel"] == DIAG, plans
    assert plans[1]["kernel"] in (_lib.SVH_KERNEL_FUSED, _lib.SVH_KERNEL_GENERIC), plans[1]
    assert plans[2]["kernel"] != DIAG and plans[3]["kernel"] == _lib.SVH_KERNEL_CHAIN, plans
    assert info["grid"] == 2 * (3 + 2), info


def test_set_sink_fed_by_feeder_runs_on_its_own():
    """A model with an N -> C edge (the sink row takes a term from the feeder row: the X_SF
    instantiations, which the set launch does not hold) keeps the diagonal plan and runs on its own."""
    h = random_chain_hmm(90, S=8, seed=411, n_from_m=False)
    h.trans_rows = np.append(h.trans_rows, np.uint64(0))
    h.trans_cols = np.append(h.trans_cols, np.uint64(91))
    h.trans_probs = np.append(h.trans_probs, np.float32(1.5))
    h.trans_num = int(h.trans_probs.size)
    hmms = [h, random_chain_hmm(90, S=8, seed=412, n_from_m=False)]
    info, fbs, plans = run_set(hmms, random_seqs(8, [100, 30], seed=11), kernels=[DIAG, DIAG])
    assert plans[0]["kernel"] == DIAG and plans[1]["kernel"] == DIAG, plans
    assert info["grouped"] == 1 and info["launches"] == 2, info


def test_set_state_across_runs_levels_and_refusals():
    """The set run twice, a member run stand-alone on its borrowed handle, the set again: arrival
    counts and flags are left clean.  Level 1 is level 0; level 2 and decoded paths are refused, so
    are an out-of-range symbol and (where the machine has two) models on two devices; a borrowed
    member cannot be destroyed."""
    hmms = [random_chain_hmm(l, S=5, seed=500 + l, n_from_m=False) for l in (40, 200, 64)]
    hmms.append(random_chain_hmm(50, S=3, seed=504, n_from_m=False))
    models = [svh.DeviceModel(h) for h in hmms]
    seqs = random_seqs(3, [150, 64, 1], seed=12)
    bs = svh.DeviceModelSet(models).batch(seqs)

    def check(tag):
        res = bs.read()
        for i, h in enumerate(hmms):
            check_member((tag, i), h, seqs, res[i][0], res[i][1])
        assert [b.fallbacks() for b in bs.members] == [0] * 4
        assert bs.info()["grouped"] == 4 and bs.info()["launches"] == 1

    bs.run()
    bs.run()
    check("twice")
    bs.members[1].run()
    s1, b1 = bs.members[1].read()
    check_member("stand-alone member", hmms[1], seqs, s1, b1)
    bs.run()
    check("after a member's own run")
    bs.run(level=1)
    check("level 1")
    assert bs.elapsed_ms() > 0
    with pytest.raises(_lib.SvhError) as e:
        bs.run(level=2)
    assert e.value.code == _lib.SVH_E_UNSUPPORTED
    assert _lib.lib.svh_batch_destroy(bs.members[0]._h) == _lib.SVH_E_INVALID
    bs.run()
    check("after the refusals")
    bs.close()
    with pytest.raises(_lib.SvhError) as e:
        svh.viterbi.DeviceBatchSet(svh.DeviceModelSet(models), seqs, paths=True)
    assert e.value.code == _lib.SVH_E_UNSUPPORTED
    with pytest.raises(_lib.SvhError) as e:  # symbol 4: inside the first three members' alphabets, outside the last's
        svh.DeviceModelSet(models).batch(random_seqs(3, [20], seed=1) + [np.array([0, 4, 1], np.uint64)])
    assert e.value.code == _lib.SVH_E_RANGE
    if _lib.device_count() >= 2:
        other = svh.DeviceModel(hmms[0], device=1)
        with pytest.raises(_lib.SvhError) as e:
            svh.DeviceModelSet([models[0], other]).batch(seqs)
        assert e.value.code == _lib.SVH_E_INVALID
        other.close()
    for m in models:
        m.close()


MODELS = sorted((os.path.basename(f) for f in os.listdir(os.path.join(DATA, "chmm_files")) if f.endswith(".chmm")),
                key=lambda f: int(f.split(".")[0]))


@pytest.fixture(scope="module")
def scope_models():
    hmms = {name: svh.read_HMM(chmm(name)) for name in MODELS}
    models = {name: svh.DeviceModel(hmms[name]) for name in MODELS}
    yield models
    for m in models.values():
        m.close()


@pytest.fixture(scope="module")
def scope_standalone(scope_models):
    """Every reference model's stand-alone emit_3 run, once for both orders."""
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    out = {}
    for name, m in scope_models.items():
        b = m.batch(seqs)
        b.run()
        out[name] = b.read()
        b.close()
    return out


@pytest.mark.parametrize("descending", [False, True])
def test_set_reference_scope(descending, scope_models, scope_standalone):
    """All 24 reference models x the three emit_3_3500_20 rows in one set, ascending and descending by
    size: 24 grouped members, one launch (about 960 workgroups), every row's score digest and best
    state as committed (tests/golden/scope_digests.json) and as the stand-alone run's, no re-run row."""
    with open(os.path.join(GOLDEN, "scope_digests.json")) as f:
        scope = json.load(f)
    assert len(MODELS) == 24
    names = MODELS[::-1] if descending else MODELS
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    bs = svh.DeviceModelSet([scope_models[n] for n in names]).batch(seqs)
    bs.run()
    res = bs.read()
    info = bs.info()
    assert info["members"] == 24 and info["grouped"] == 24 and info["launches"] == 1 and info["waves"] == 2, info
    ranges = [-(-(scope_models[n].n - 2) // 64) for n in names]
    assert info["grid"] == 2 * sum(ranges), (info, sum(ranges))
    for i, name in enumerate(names):
        ref = scope["models"][name]
        scores, best = res[i]
        for q in range(len(seqs)):
            digest = hashlib.sha256(np.ascontiguousarray(scores[q], np.float32).tobytes()).hexdigest()
            assert digest == ref[q]["scores_sha256"], (name, q)
            assert int(best[q]) == ref[q]["best_state"], (name, q, int(best[q]))
            assert bit_equal(scores[q], scope_standalone[name][0][q]), (name, q, "stand-alone")
        assert np.array_equal(best, scope_standalone[name][1]), name
        assert bs.members[i].plan()["kernel"] == DIAG
        assert bs.members[i].fallbacks() == 0, name
    bs.close()
