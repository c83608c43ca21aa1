"""`_spec` level 2 on the diagonal plan (diag_l2.hip, SVH_KERNEL_SPEC2_DIAG): models created with
SVH_KERNEL_DIAG run every chunk of two observations of every row in one launch, a lane advancing two
positions per chunk; rows whose speculation fails are re-run by spec2_kernel.

A fallback hides a wrong row, so every geometry test asserts that no row fell back; that its inputs
cannot fall back is established without a device by tests/test_diag_l2_cases.py."""
import hashlib

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.conftest import chmm, ess
from tests.diag_l2_cases import (CHUNKS_PER_BLOCK, EDGE_VARIANTS, FALLBACK_CASES, FILL_ROWS, NO_FALLBACK_CASES, RANGE_SIZES,
                                 inf_feeder)
from tests.helpers import bit_equal, first_mismatch, load_digests, random_chain_hmm, random_seqs

pytestmark = pytest.mark.gpu

DIAG = _lib.SVH_KERNEL_DIAG
L2DIAG = _lib.SVH_KERNEL_SPEC2_DIAG


def _run_case(name):
    """One case of NO_FALLBACK_CASES on the route: bit-exact against the oracle, no row re-run."""
    case = NO_FALLBACK_CASES[name]
    hmm, seqs = case.build(), case.seqs()
    model = svh.DeviceModel(hmm, kernel=DIAG)
    model.spec_build(2)
    batch = model.batch(seqs)
    plan = batch.plan(2)
    assert plan["kernel"] == L2DIAG, plan["kernel"]
    w = 4 if len(seqs) >= 4 else 2 if len(seqs) >= 2 else 1
    assert plan["threads"] == 64 * w and plan["slots"] == 1 and plan["spec_bytes"] == 0 and plan["lds_bytes"] > 0
    batch.run(2)
    got, _ = batch.read()
    flags = batch.fallback_rows()
    batch.close()
    model.close()
    assert not flags.any(), (name, flags)
    refs = oracle.viterbi_spec_batch(hmm, 2, seqs)
    for q in range(len(seqs)):
        assert bit_equal(got[q], refs[q]), (name, q, len(seqs[q]), first_mismatch(got[q], refs[q]))


def test_lengths():
    """L = 100 (two ranges, NP = 128), S = 8: 0 .. 5 B + 1 chunks around the block length B with
    both tail parities, and a row of more than 2 NP chunks (every lane wraps four times)."""
    _run_case("lengths")


@pytest.mark.parametrize("L", RANGE_SIZES)
def test_ranges(L):
    """One range with dummies, a full range, dummy positions directly ahead of the wrap."""
    _run_case(f"range{L}")


@pytest.mark.parametrize("rows", FILL_ROWS)
def test_workgroup_fill(rows):
    """A partial last workgroup, idle waves, every workgroup width the launcher picks."""
    _run_case(f"fill{rows}")


@pytest.mark.parametrize("variant", list(EDGE_VARIANTS))
def test_edge_values(variant):
    """Exact ties, +inf edges and emissions, a chain break, a start inside the chain."""
    _run_case(f"edge_{variant}")


def _digest_bad(got, rows):
    return [q for q in range(len(rows))
            if hashlib.sha256(np.ascontiguousarray(got[q], np.float32).tobytes()).hexdigest() != rows[q]["scores_sha256"]]


def test_reference_data_all_rows_twice():
    """2405.chmm x emit_50, all 50 rows against the oracle's level-2 digests, the same batch object
    run twice (arrival counts, the flags of the last run), no row re-run."""
    hmm = svh.read_HMM(chmm("2405.chmm"))
    seqs = svh.read_emit_seq(ess("emit_50_3500_20.ess"))
    rows = load_digests()["2405.chmm x emit_50_3500_20.ess level 2"]
    model = svh.DeviceModel(hmm, kernel=DIAG)
    model.spec_build(2)
    batch = model.batch(seqs)
    assert batch.plan(2)["kernel"] == L2DIAG
    for _ in range(2):
        batch.run(2)
        got, best = batch.read()
        assert batch.fallbacks() == 0
        assert not batch.fallback_rows().any()
        assert not _digest_bad(got, rows)
        assert np.array_equal(best, np.argmin(got, axis=1))
    batch.close()
    model.close()


def test_reference_data_ragged_prefixes_equal_pipe_l2():
    """Prefixes of four reference rows across block boundaries (a block is 32 chunks), bit-equal to
    the same batch on an AUTO model, where the pipelined level-2 kernel is the second witness."""
    B = CHUNKS_PER_BLOCK
    hmm = svh.read_HMM(chmm("2405.chmm"))
    base = svh.read_emit_seq(ess("emit_50_3500_20.ess"))
    seqs = [base[3][:2 * B + 1], base[11][:2 * B + 2], base[29][:2 * (3 * B + 1) + 2], base[47][:2 * (7 * B - 1) + 1]]
    out = {}
    for kern, want in ((DIAG, L2DIAG), (_lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_SPEC2_PIPE)):
        model = svh.DeviceModel(hmm, kernel=kern)
        model.spec_build(2)
        batch = model.batch(seqs)
        assert batch.plan(2)["kernel"] == want
        batch.run(2)
        out[kern] = batch.read()
        assert not batch.fallback_rows().any()
        batch.close()
        model.close()
    for q in range(len(seqs)):
        assert bit_equal(out[DIAG][0][q], out[_lib.SVH_KERNEL_AUTO][0][q]), q
    assert np.array_equal(out[DIAG][1], out[_lib.SVH_KERNEL_AUTO][1])


@pytest.mark.parametrize("n_states", [300, 1300])
def test_flagged_rows_match_oracle_and_pipe_l2(n_states):
    """M -> N free: rows fail the check and spec2_kernel re-runs them.  Every row equals the oracle
    bit for bit, and the rows handed over are those the pipelined level-2 pass hands over."""
    total = 0
    for seed in range(3):
        case = FALLBACK_CASES[f"free{n_states}_{seed}"]
        hmm, seqs = case.build(), case.seqs()
        flags = {}
        for kern, want in ((DIAG, L2DIAG), (_lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_SPEC2_PIPE)):
            model = svh.DeviceModel(hmm, kernel=kern)
            model.spec_build(2)
            batch = model.batch(seqs)
            assert batch.plan(2)["kernel"] == want
            batch.run(2)
            got, _ = batch.read()
            flags[kern] = batch.fallback_rows() & 2
            if kern == DIAG:
                total += batch.fallbacks()
                refs = oracle.viterbi_spec_batch(hmm, 2, seqs)
                for q in range(len(seqs)):
                    assert bit_equal(got[q], refs[q]), (seed, q, first_mismatch(got[q], refs[q]))
            batch.close()
            model.close()
        assert np.array_equal(flags[DIAG], flags[_lib.SVH_KERNEL_AUTO]), (seed, flags)
    assert total > 0


def _plan2(hmm, kernel=DIAG, flags=0):
    model = svh.DeviceModel(hmm, kernel=kernel, flags=flags)
    model.spec_build(2)
    batch = model.batch(random_seqs(int(hmm.emit_num), [9, 40], seed=1))
    p2, p0 = batch.plan(2), batch.plan(0)
    batch.close()
    model.close()
    return p2, p0


def test_route_guards():
    """Models the route does not take keep today's: a negative score (emax2), more than 32 symbols,
    the dense products; kernel 10 cannot be selected; level 0 of the same batch stays on DIAG."""
    hmm = inf_feeder(random_chain_hmm(100, S=8, seed=41))
    p2, p0 = _plan2(hmm)
    assert p2["kernel"] == L2DIAG and p0["kernel"] == DIAG
    # a negative score: the margin bound does not hold, spec2_kernel runs every chunk
    neg = inf_feeder(random_chain_hmm(100, S=8, seed=41))
    tp = neg.trans_probs.copy()
    n_to_m = np.flatnonzero((neg.trans_rows == 0) & (neg.trans_cols != 0))  # (the shared weights stay uniform)
    tp[n_to_m[::3]] *= np.float32(-0.5)
    neg.trans_probs = tp
    assert _plan2(neg)[0]["kernel"] == _lib.SVH_KERNEL_SPEC2
    # 33 symbols: no diagonal table, so the model cannot be created with SVH_KERNEL_DIAG at all; under
    # AUTO it keeps spec2_kernel
    wide = inf_feeder(random_chain_hmm(100, S=33, seed=42))
    with pytest.raises(_lib.SvhError):
        svh.DeviceModel(wide, kernel=DIAG)
    assert _plan2(wide, kernel=_lib.SVH_KERNEL_AUTO)[0]["kernel"] == _lib.SVH_KERNEL_SPEC2
    # the dense products stay what SVH_MODEL_SPEC_DENSE asks for
    pd, _ = _plan2(hmm, flags=_lib.SVH_MODEL_SPEC_DENSE)
    assert pd["kernel"] not in (L2DIAG, _lib.SVH_KERNEL_SPEC2, _lib.SVH_KERNEL_SPEC2_PIPE) and pd["spec_bytes"] > 0
    # reported only, never selected
    with pytest.raises(_lib.SvhError) as e:
        svh.DeviceModel(hmm, kernel=L2DIAG)
    assert e.value.code == _lib.SVH_E_INVALID


def test_sink_fed_by_feeder_keeps_spec2_kernel():
    """A model whose sink row takes a term from the feeder (N -> C) is left out of the route: its
    level-2 chunks stay on spec2_kernel, bit-exact."""
    hmm = inf_feeder(random_chain_hmm(100, S=8, seed=43))
    C = int(hmm.states_num) - 1
    hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))
    hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(C))
    hmm.trans_probs = np.append(hmm.trans_probs, np.float32(2.5))
    hmm.trans_num = int(hmm.trans_probs.size)
    seqs = random_seqs(8, [1, 2, 9, 70, 131], seed=43)
    model = svh.DeviceModel(hmm, kernel=DIAG)
    model.spec_build(2)
    batch = model.batch(seqs)
    assert batch.plan(0)["kernel"] == DIAG
    assert batch.plan(2)["kernel"] == _lib.SVH_KERNEL_SPEC2
    batch.run(2)
    got, _ = batch.read()
    batch.close()
    model.close()
    refs = oracle.viterbi_spec_batch(hmm, 2, seqs)
    for q in range(len(seqs)):
        assert bit_equal(got[q], refs[q]), (q, first_mismatch(got[q], refs[q]))


def test_shared_batch_object_levels_0_2_0():
    """One model, one batch: level 0, level 2, level 0 again, each bit-exact (the shared scratch,
    the level-2 buffers' readiness key)."""
    case = NO_FALLBACK_CASES["lengths"]
    hmm, seqs = case.build(), case.seqs()
    ref0 = [oracle.viterbi(hmm, s) for s in seqs]
    ref2 = oracle.viterbi_spec_batch(hmm, 2, seqs)
    model = svh.DeviceModel(hmm, kernel=DIAG)
    model.spec_build(2)
    batch = model.batch(seqs)
    assert batch.plan(2)["kernel"] == L2DIAG and batch.plan(0)["kernel"] == DIAG
    for level, refs in ((0, ref0), (2, ref2), (0, ref0)):
        batch.run(level)
        got, _ = batch.read()
        for q in range(len(seqs)):
            assert bit_equal(got[q], refs[q]), (level, q, first_mismatch(got[q], refs[q]))
    batch.close()
    model.close()


def test_python_spec_impl_reaches_the_route():
    """HIP_spec_impl(2, kernel=SVH_KERNEL_DIAG) runs on the route through its model options."""
    case = NO_FALLBACK_CASES["edge_start"]
    hmm, seqs = case.build(), case.seqs()
    impl = svh.HIP_spec_impl(2, kernel=DIAG)
    impl.spec_with(hmm)
    assert impl._model.batch(seqs[:1]).plan(2)["kernel"] == L2DIAG
    got = impl.run_Viterbi_spec_batch(seqs)
    refs = oracle.viterbi_spec_batch(hmm, 2, seqs)
    for q in range(len(seqs)):
        assert bit_equal(got[q], refs[q]), (q, first_mismatch(got[q], refs[q]))
