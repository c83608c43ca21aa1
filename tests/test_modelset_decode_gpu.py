"""GPU parity of a model set's decode pass (svh_batchset_decode, DeviceBatchSet.decode): the state
paths of chosen (member, row) pairs, the members whose path plan is the diagonal path variant in ONE
forward launch (diag.hip diag_set_paths_kernel) and ONE traceback launch (pipe_paths.hip
diag_set_traceback_kernel), each workgroup finding its member from its block index.

Every case compares each pair's scores bit for bit, its best state and every path entry with
oracle.decode(hmm, seq), and asserts how many members the set's launches took (`grouped`) and how many
launches the decode made.  A row whose speculation fails is decoded by the chain path variant, which
would also hide a wrong diagonal record: models without M -> N terms (n_from_m=False) cannot fail it,
and those cases assert fallback_pairs == 0; the fallback case asserts which member's rows did.
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
from tests.helpers import (GOLDEN, bit_equal, first_mismatch, random_chain_hmm, random_hmm, random_seqs,
                           relabel_chain_hmm)

pytestmark = pytest.mark.gpu
DIAG = _lib.SVH_KERNEL_DIAG
AUTO = _lib.SVH_KERNEL_AUTO


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def waves_for(nseq):
    return 4 if nseq >= 4 else 2 if nseq >= 2 else 1


def paths_lds(W, S):
    """The path variant's LDS without an X_SF stream (diag_launch.h diag_lds_paths): the scores layout
    -- ring [S][320 + 64] float2, symbol template [S][8], constants and ring addresses [W][2][64] x 5
    floats, 2 W words -- rounded up to 16 bytes, then the fold ring [W][8][64] floats."""
    main = (S * 384 * 2 + S * 8 + W * 2 * 64 * 5 + 2 * W) * 4
    return ((main + 15) & ~15) + W * 8 * 64 * 4


def paths_fit(S):
    """diag_launch.h diag_paths_fit: the widest workgroup's footprint leaves room for two on a CU."""
    return S <= 32 and paths_lds(4, S) <= 80 * 1024


def free_feeder(hmm, weight):
    """M_j -> N at `weight` for every j (0: N takes its light term, the speculation fails; +inf: never)."""
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    probs = hmm.trans_probs.copy()
    probs[(cols == 0) & (rows != 0)] = np.float32(weight)
    hmm.trans_probs = probs
    return hmm


class Refs:
    """oracle.decode(hmm_i, seq_r), computed once per (member, row) and left unchanged."""

    def __init__(self, hmms, seqs):
        self.hmms, self.seqs, self.memo = hmms, seqs, {}

    def __call__(self, m, r):
        if (m, r) not in self.memo:
            self.memo[(m, r)] = oracle.decode(self.hmms[m], self.seqs[r])
        return self.memo[(m, r)]


def check_pairs(tag, refs, pairs, got, first=()):
    """Every pair of a decode against the oracle (the pairs of the members in `first` first)."""
    order = sorted(range(len(pairs)), key=lambda k: (pairs[k][0] not in first, k))
    assert len(got) == len(pairs), (tag, len(got), len(pairs))
    for k in order:
        m, r = pairs[k]
        ref, ref_best, ref_path = refs(m, r)
        scores, best, path = got[k][:3]
        assert bit_equal(scores, ref), (tag, k, m, r, first_mismatch(scores, ref))
        assert best == ref_best, (tag, k, m, r, best, ref_best)
        assert path.shape == ref_path.shape and np.array_equal(path, ref_path), (tag, k, m, r, np.nonzero(path != ref_path)[0][:5])


def check_standalone(tag, models, seqs, pairs, got):
    """Every pair against a stand-alone path batch of its model over the member's chosen rows."""
    for m in sorted({p[0] for p in pairs}):
        ks = [k for k, p in enumerate(pairs) if p[0] == m]
        b = models[m].batch([seqs[pairs[k][1]] for k in ks], paths=True)
        b.run()
        s1, b1, p1 = b.read(want_paths=True)
        b.close()
        for j, k in enumerate(ks):
            assert bit_equal(got[k][0], s1[j]), (tag, "stand-alone", k)
            assert got[k][1] == int(b1[j]) and np.array_equal(got[k][2], p1[j]), (tag, "stand-alone path", k)


def grid_of(pairs, nrng, members, W):
    """sum over the grouped members of ceil(chosen rows / W) x ranges."""
    return sum(-(-sum(1 for p in pairs if p[0] == i) // W) * nrng[i] for i in members if any(p[0] == i for p in pairs))


def make_set(hmms, seqs, kernels=None, timing=True):
    kernels = kernels or [DIAG] * len(hmms)
    models = [svh.DeviceModel(h, kernel=k) for h, k in zip(hmms, kernels)]
    return models, svh.DeviceModelSet(models).batch(seqs, timing=timing)


def close_all(bs, models):
    bs.close()
    for m in models:
        m.close()


@pytest.mark.parametrize("rev", [False, True])
def test_decode_entry_lookup_edges(rev):
    """Members of 1, 1, 1, 2 and 3 ranges (1, 63, 64, 65, 129 light rows), in that order and reversed:
    every first[] boundary of both tables has a one-block neighbour.  Pair lists with every pair, one
    pair at either end, the middle members left out, 1 .. 5 rows per member (idle waves at every W)
    and one pair twice."""
    L = [1, 63, 64, 65, 129]
    L = L[::-1] if rev else L
    hmms = [random_chain_hmm(l, S=20, seed=10 + l, n_from_m=False) for l in L]
    nrng = [-(-l // 64) for l in L]
    seqs = random_seqs(20, [1, 2, 64, 65, 130], seed=5)
    refs = Refs(hmms, seqs)
    models, bs = make_set(hmms, seqs)
    lists = {
        "every pair": [(m, r) for m in range(5) for r in range(5)],
        "first member": [(0, 3)],
        "last member": [(4, 4)],
        "middle left out": [(0, 0), (4, 2), (0, 4), (4, 1), (0, 2)],
        "1..5 rows per member": [(m, r) for m in range(5) for r in range(m + 1)],
        "one pair twice": [(2, 4), (1, 1), (2, 4)],
    }
    for tag, pairs in lists.items():
        bs.decode(pairs)
        got = bs.read_decoded(fell_back=True)
        check_pairs(tag, refs, pairs, got)
        if tag in ("every pair", "one pair twice"):
            check_standalone(tag, models, seqs, pairs, got)
        info = bs.decode_info()
        per = [sum(1 for p in pairs if p[0] == i) for i in range(5)]
        W = waves_for(max(per))
        assert info["pairs"] == len(pairs) and info["members"] == sum(1 for c in per if c), (tag, info)
        assert info["grouped"] == info["members"] and info["grouped_pairs"] == len(pairs), (tag, info)
        assert info["waves"] == W and info["grid"] == grid_of(pairs, nrng, range(5), W), (tag, info)
        assert info["launches"] == 2 + 2 * info["grouped"], (tag, info)
        assert info["fallback_pairs"] == 0 and not any(g[3] for g in got), (tag, info)
    close_all(bs, models)


def test_decode_record_edges():
    """Two members (300 and 700 light rows), rows at the records' edges -- the fold every 8 steps, the
    words and checkpoints every 32, the 64-step block, one turn of the 320-column ring -- split over
    two decodes of one set."""
    hmms = [random_chain_hmm(300, S=20, seed=31, n_from_m=False), random_chain_hmm(700, S=20, seed=32, n_from_m=False)]
    lens = [1, 8, 9, 31, 32, 33, 63, 64, 65, 129, 321]
    seqs = random_seqs(20, lens, seed=33)
    refs = Refs(hmms, seqs)
    models, bs = make_set(hmms, seqs)
    for half in (0, 1):
        pairs = [(m, r) for r in range(len(lens)) for m in (0, 1) if (r + m) % 2 == half]
        bs.decode(pairs)
        check_pairs(half, refs, pairs, bs.read_decoded())
        info = bs.decode_info()
        assert info["grouped"] == 2 and info["grouped_pairs"] == len(pairs) and info["fallback_pairs"] == 0, info
        assert info["waves"] == 4 and info["launches"] == 6, info
    close_all(bs, models)


def test_decode_more_than_64_entries():
    """70 members of 3 .. 72 light rows, 1 + (i mod 3) rows chosen of member i: the lookup's second
    chunk of 64 entries in a traceback table that is not uniform; members 0, 63, 64 and 69 first."""
    hmms = [random_chain_hmm(3 + i, S=6, seed=200 + i, n_from_m=False) for i in range(70)]
    seqs = random_seqs(6, [70, 70, 70], seed=7)
    pairs = [(i, (i + j) % 3) for i in range(70) for j in range(1 + i % 3)]
    models, bs = make_set(hmms, seqs)
    bs.decode(pairs)
    check_pairs("70", Refs(hmms, seqs), pairs, bs.read_decoded(), first=(0, 63, 64, 69))
    info = bs.decode_info()
    assert info["members"] == 70 and info["grouped"] == 70 and info["grouped_pairs"] == len(pairs), info
    assert info["waves"] == 2 and info["launches"] == 2 + 140 and info["fallback_pairs"] == 0, info
    assert info["grid"] == sum(-(-(1 + i % 3) // 2) * -(-(3 + i) // 64) for i in range(70)), info
    close_all(bs, models)


def test_decode_alphabets_and_lds():
    """Members of 3, 20 and 32 symbols (sequences over the first 3): each workgroup lays its LDS out for
    its own alphabet, the launch asks for the largest grouped member's path footprint.  The path variant
    takes a model whose widest workgroup leaves room for two on a CU (diag_paths_fit): by the formula
    restated above that holds for 3 and 20 symbols and not for 32, whose decode batch runs on its own."""
    S = (3, 20, 32)
    hmms = [random_chain_hmm(100, S=s, seed=300 + s, n_from_m=False) for s in S]
    seqs = random_seqs(3, [200, 65], seed=8)
    pairs = [(m, r) for m in range(3) for r in range(2)]
    fit = [s for s in S if paths_fit(s)]
    assert fit == [3, 20]
    models, bs = make_set(hmms, seqs)
    bs.decode(pairs)
    check_pairs("alphabets", Refs(hmms, seqs), pairs, bs.read_decoded())
    info = bs.decode_info()
    assert info["members"] == 3 and info["grouped"] == len(fit) and info["grouped_pairs"] == 2 * len(fit), info
    assert info["waves"] == 2 and info["grid"] == 2 * len(fit), info
    assert info["lds_bytes"] == paths_lds(2, max(fit)), (info, paths_lds(2, max(fit)))
    assert info["launches"] == 2 + 2 * len(fit) + (3 - len(fit)) and info["fallback_pairs"] == 0, info
    close_all(bs, models)


def test_decode_fallback_sees_its_own_member():
    """A member whose feeder row takes its light term (M -> N free) between two whose M -> N weight is
    +inf, over the seeds and length sets of test_modelset_gpu.py's re-run case: the chain path variant
    and both tracebacks must run with the middle member's model, batch and flags.  Only the middle
    member's pairs report a fallback, over the seeds at least one, and every path is exact."""
    middle = 0
    for seed in range(8):
        n = 300 if seed < 6 else 700
        hmms = [free_feeder(random_chain_hmm(n - 37, S=8, seed=50 + seed), np.inf),
                free_feeder(random_chain_hmm(n, S=8, seed=seed), 0.0),
                free_feeder(random_chain_hmm(n + 70, S=8, seed=90 + seed), np.inf)]
        lens = [[700], [700, 1], [700, 1, 40, 333, 64]][seed % 3]
        seqs = random_seqs(8, lens, seed=seed)
        pairs = [(m, r) for r in range(len(lens)) for m in range(3)]
        models, bs = make_set(hmms, seqs)
        bs.decode(pairs)
        got = bs.read_decoded(fell_back=True)
        check_pairs(seed, Refs(hmms, seqs), pairs, got)
        if seed % 3 == 2:
            check_standalone(seed, models, seqs, pairs, got)
        info = bs.decode_info()
        assert info["grouped"] == 3 and info["launches"] == 8, (seed, info)
        fell = [k for k, g in enumerate(got) if g[3]]
        assert all(pairs[k][0] == 1 for k in fell), (seed, fell)
        assert info["fallback_pairs"] == len(fell), (seed, info, fell)
        middle += len(fell)
        close_all(bs, models)
    assert middle > 0


def test_decode_mixed_eligibility():
    """Beside two grouped members: a chain model created with AUTO (its path batches stay on the
    pipelined variant), a general model, a SVH_KERNEL_CHAIN model, a SVH_KERNEL_DIAG model with an
    N -> C edge (X_SF) and a relabelled one whose N does not win ties.  Two members in the set's
    launches, five runs of their own after them, every member exact."""
    sx = random_chain_hmm(90, S=12, seed=411, n_from_m=False)
    sx.trans_rows = np.append(sx.trans_rows, np.uint64(0))
    sx.trans_cols = np.append(sx.trans_cols, np.uint64(91))
    sx.trans_probs = np.append(sx.trans_probs, np.float32(1.5))
    sx.trans_num = int(sx.trans_probs.size)
    late_n, _ = relabel_chain_hmm(random_chain_hmm(80, S=12, seed=406, n_from_m=False), 81, 0)
    hmms = [random_chain_hmm(150, S=12, seed=401, n_from_m=False), random_chain_hmm(120, S=12, seed=407, n_from_m=False),
            random_hmm(200, S=12, seed=402), random_chain_hmm(140, S=12, seed=404, n_from_m=False), sx, late_n,
            random_chain_hmm(70, S=12, seed=405, n_from_m=False)]
    kernels = [DIAG, AUTO, AUTO, _lib.SVH_KERNEL_CHAIN, DIAG, DIAG, DIAG]
    seqs = random_seqs(12, [130, 64, 3], seed=9)
    pairs = [(m, r) for m in range(7) for r in range(3) if (m + r) % 4 != 3]
    models, bs = make_set(hmms, seqs, kernels)
    bs.decode(pairs)
    got = bs.read_decoded()
    check_pairs("mixed", Refs(hmms, seqs), pairs, got)
    check_standalone("mixed", models, seqs, pairs, got)
    info = bs.decode_info()
    assert info["members"] == 7 and info["grouped"] == 2, info
    assert info["grouped_pairs"] == sum(1 for p in pairs if p[0] in (0, 6)), info
    assert info["launches"] == 2 + 2 * 2 + 5, info
    W = waves_for(max(sum(1 for p in pairs if p[0] == i) for i in (0, 6)))
    assert info["waves"] == W and info["grid"] == grid_of(pairs, {0: 3, 6: 2}, (0, 6), W), info
    close_all(bs, models)


def test_decode_state_and_refusals():
    """Decodes between, before and after scores runs leave the members' scores state alone; a repeated
    list builds nothing; a set without timing decodes; two sets decode on two streams; the error codes."""
    import torch

    hmms = [random_chain_hmm(l, S=5, seed=500 + l, n_from_m=False) for l in (40, 200, 64)]
    seqs = random_seqs(5, [150, 64, 1], seed=12)
    refs = Refs(hmms, seqs)
    every = [(m, r) for m in range(3) for r in range(3)]
    other = [(2, 0), (0, 1), (2, 0)]
    models, bs = make_set(hmms, seqs)

    def scores_exact(tag, res):
        for i in range(3):
            for q in range(3):
                assert bit_equal(res[i][0][q], refs(i, q)[0]) and int(res[i][1][q]) == refs(i, q)[1], (tag, i, q)

    with pytest.raises(_lib.SvhError) as e:  # a read before any decode
        bs.read_decoded()
    assert e.value.code == _lib.SVH_E_STATE
    assert bs.decode_info()["builds"] == 0
    bs.run()
    res0 = bs.read()
    scores_exact("run", res0)
    plans0 = [b.plan() for b in bs.members]
    bs.decode(every)
    check_pairs("after a run", refs, every, bs.read_decoded())
    res1 = bs.read()
    for i in range(3):
        assert np.array_equal(res0[i][0].view(np.uint32), res1[i][0].view(np.uint32)) and np.array_equal(res0[i][1], res1[i][1]), i
    assert [b.fallbacks() for b in bs.members] == [0] * 3 and [b.plan() for b in bs.members] == plans0
    assert bs.info()["launches"] == 1 and bs.info()["grouped"] == 3

    # the same list twice: equal results, nothing rebuilt; another list, then the first again
    first = bs.read_decoded()
    builds = bs.decode_info()["builds"]
    bs.decode(every)
    again = bs.read_decoded()
    assert bs.decode_info()["builds"] == builds
    for a, b in zip(first, again):
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1] and np.array_equal(a[2], b[2])
    bs.decode(other)
    check_pairs("another list", refs, other, bs.read_decoded())
    assert bs.decode_info()["builds"] == builds + 1 and bs.decode_info()["pairs"] == 3
    bs.decode(every)
    check_pairs("the first again", refs, every, bs.read_decoded())
    assert bs.decode_info()["builds"] == builds + 2
    assert bs.decode_elapsed_ms() > 0
    bs.run()
    scores_exact("run after decodes", bs.read())

    # refusals leave the last decode readable
    for bad in ([(3, 0)], [(0, 3)], [(0, 0), (1, 7)]):
        with pytest.raises(_lib.SvhError) as e:
            bs.decode(bad)
        assert e.value.code == _lib.SVH_E_RANGE, bad
    with pytest.raises(_lib.SvhError) as e:
        bs.decode([])
    assert e.value.code == _lib.SVH_E_INVALID
    check_pairs("after the refusals", refs, every, bs.read_decoded())
    with pytest.raises(_lib.SvhError) as e:  # unchanged: no SVH_BATCH_PATHS at create
        svh.viterbi.DeviceBatchSet(svh.DeviceModelSet(models), seqs, paths=True)
    assert e.value.code == _lib.SVH_E_UNSUPPORTED

    # a fresh set: a decode before any run; without timing: no decode events
    fresh = svh.DeviceModelSet(models).batch(seqs, timing=False)
    fresh.decode(other)
    check_pairs("fresh set", refs, other, fresh.read_decoded())
    with pytest.raises(_lib.SvhError) as e:
        fresh.decode_elapsed_ms()
    assert e.value.code == _lib.SVH_E_STATE
    fresh.run()
    scores_exact("fresh set's run", fresh.read())

    # two sets, two streams
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        bs.decode(every, sa.cuda_stream)
        fresh.decode(every[::-1], sb.cuda_stream)
        check_pairs("stream a", refs, every, bs.read_decoded(sa.cuda_stream))
        check_pairs("stream b", refs, every[::-1], fresh.read_decoded(sb.cuda_stream))
    fresh.close()
    close_all(bs, models)


MODELS = sorted((os.path.basename(f) for f in os.listdir(os.path.join(DATA, "chmm_files")) if f.endswith(".chmm")),
                key=lambda f: int(f.split(".")[0]))


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype)).tobytes()).hexdigest()


def test_decode_reference_scope():
    """All 24 reference models, created with SVH_KERNEL_DIAG, x the three emit_3_3500_20 rows: 72 pairs
    in one decode, every row's scores, best state and path digest as committed
    (tests/golden/scope_digests.json), 24 grouped members, no fallback; then 2405.chmm's pairs alone."""
    with open(os.path.join(GOLDEN, "scope_digests.json")) as f:
        scope = json.load(f)["models"]
    assert len(MODELS) == 24
    seqs = svh.read_emit_seq(ess("emit_3_3500_20.ess"))
    models = [svh.DeviceModel(svh.read_HMM(chmm(name)), kernel=DIAG) for name in MODELS]
    bs = svh.DeviceModelSet(models).batch(seqs)

    def check(pairs):
        bs.decode(pairs)
        for (m, r), (scores, best, path) in zip(pairs, bs.read_decoded()):
            ref = scope[MODELS[m]][r]
            assert sha(scores, np.float32) == ref["scores_sha256"], (MODELS[m], r)
            assert best == ref["best_state"], (MODELS[m], r, best)
            assert sha(path, np.int32) == ref["path_sha256"], (MODELS[m], r)
        return bs.decode_info()

    info = check([(m, r) for m in range(24) for r in range(3)])
    assert info["pairs"] == 72 and info["grouped"] == 24 and info["grouped_pairs"] == 72 and info["fallback_pairs"] == 0, info
    assert info["waves"] == 2 and info["launches"] == 2 + 48, info
    assert info["grid"] == 2 * sum(-(-(m.n - 2) // 64) for m in models), info
    last = MODELS.index("2405.chmm")
    info = check([(last, r) for r in range(3)])
    assert info["pairs"] == 3 and info["grouped"] == 1 and info["fallback_pairs"] == 0 and info["launches"] == 4, info
    close_all(bs, models)
