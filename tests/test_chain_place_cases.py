"""The inputs of tests/test_chain_place_gpu.py, checked without a device (tests/chain_place_cases.py).

The GPU tests run chain-shaped models whose feeder row N and sink row C were moved to other state
indices.  What they rely on is a property of the models and the sequences, so it is established here
with the oracle alone: the relabelled model is the same model (scores bit for bit at the moved
indices); its tie outcomes are not (decoded paths and best states differ from the relabelled
control's); the families whose GPU tests assert zero fallbacks never fail the speculation check, family
B ties the feeder's light term with its self term on the way, and family C does fail it."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests.chain_place_cases import CASES, PLAN_L, build, names, placed, placements, seqs
from tests.helpers import bit_equal, chain_speculation, first_mismatch

SIZES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def decoded(L, name, place):
    """The oracle's (scores, best state, path) per row of one case at one placement."""
    hmm2, _, _ = placed(CASES[L][name], place)
    return [oracle.decode(hmm2, s) for s in seqs(CASES[L][name])]


@functools.lru_cache(maxsize=None)
def speculation(L, name):
    case = CASES[L][name]
    hmm = build(case)
    return [chain_speculation(hmm, s) for s in seqs(case)]


def test_sizes_and_placements():
    assert set(PLAN_L.values()) == set(SIZES)
    for L in SIZES:
        assert placements(L)[0] == (0, L + 1)
        assert all(len(c.lengths) <= 6 and max(c.lengths) <= 300 for c in CASES[L].values())
        assert {c.family for c in CASES[L].values()} == set("ABCDE")


def test_planner_takes_n_and_c_at_any_index():
    """The chain planner (runtime.cpp band_heavy_rows, make_band_plan, make_pipe_plan) through the
    stand-alone program tests/cpp/test_chain_place.cpp, built with AddressSanitizer + UBSan: with
    and without M -> N terms, every placement is planned with F = N, S = C and the light rows in
    chain order.  Nothing is loaded into Python and no GPU is touched."""
    import os
    import subprocess

    from tests.conftest import ROOT

    prog = os.path.join(ROOT, "tests", "cpp", "test_chain_place")
    assert os.path.exists(prog), "tests/cpp/test_chain_place not built (make tests)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([prog], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "36 models, 0 failures" in r.stdout and "ok" in r.stdout, r.stdout


def test_relabel_moves_indices_only():
    """The control placement is the identity; elsewhere new[] is a permutation that keeps the light
    rows in order, and every weight, the tuple order and the emission columns are the control's."""
    L = SIZES[0]
    case = CASES[L]["B"]
    for place in placements(L):
        hmm2, new, hmm = placed(case, place)
        assert sorted(new) == list(range(L + 2)) and (new[0], new[L + 1]) == place
        assert np.all(np.diff(new[1:L + 1]) > 0)
        assert np.array_equal(hmm2.trans_probs.view(np.uint32), hmm.trans_probs.view(np.uint32))
        assert np.array_equal(hmm2.trans_rows, new[hmm.trans_rows.astype(np.int64)])
        assert np.array_equal(hmm2.trans_cols, new[hmm.trans_cols.astype(np.int64)])
        assert np.array_equal(hmm2.emissions[:, new].view(np.uint32), hmm.emissions.view(np.uint32))
        assert np.array_equal(hmm2.start_probabilities_cols, new[hmm.start_probabilities_cols.astype(np.int64)])
        if place == (0, L + 1):
            assert np.array_equal(new, np.arange(L + 2)) and np.array_equal(hmm2.emissions, hmm.emissions)


@pytest.mark.parametrize("L", SIZES)
def test_relabelled_scores_are_the_controls(L):
    """Every case and placement: the oracle's scores of the relabelled model equal the control's at
    new[...], bit for bit, and some are finite."""
    for name, case in CASES[L].items():
        control = decoded(L, name, placements(L)[0])
        for place in placements(L)[1:]:
            _, new, _ = placed(case, place)
            for q, ((s2, _, _), (s0, _, _)) in enumerate(zip(decoded(L, name, place), control)):
                assert bit_equal(s2[new], s0), (name, place, q, first_mismatch(s2[new], s0))
        assert sum(int(np.isfinite(s).sum()) for s, _, _ in control) > 0, name


@pytest.mark.parametrize("which", range(1, 6))
def test_ties_resolve_differently(which):
    """Every placement but the control, summed over its family A and B cases: decoded-path entries and
    best states differ from the control's mapped through new[...]."""
    paths = bests = 0
    for L in SIZES:
        place = placements(L)[which]
        for name in names(L, "AB"):
            _, new, _ = placed(CASES[L][name], place)
            for (_, b2, p2), (_, b0, p0) in zip(decoded(L, name, place), decoded(L, name, placements(L)[0])):
                paths += int((p2 != new[p0]).sum())
                bests += int(b2 != new[b0])
    assert paths >= 1 and bests >= 1, (which, paths, bests)


@pytest.mark.parametrize("L", SIZES)
def test_no_fallback_families_pass_the_check(L):
    """Families A, D and E (F has no light term) and B (its light term ties, never wins): no row
    fails the check, so the GPU tests may assert that none fell back."""
    for name in names(L, "ABDE"):
        assert all(t == -1 for t, _ in speculation(L, name)), (name, speculation(L, name))


@pytest.mark.parametrize("L", SIZES)
def test_family_b_ties_and_enters_n_from_a_light_row(L):
    """Family B: at least half the rows of every case meet a tied feeder term, and with N above the
    light rows the oracle's path holds an entry whose state is N and whose previous state is a light
    row (the backpointer the strict check leaves to the tie rule)."""
    for name in names(L, "B"):
        spec = speculation(L, name)
        assert 2 * sum(k >= 1 for _, k in spec) >= len(spec), (name, spec)
        for place in placements(L):
            n_at, c_at = place
            if n_at != L + 1:
                continue
            entries = 0
            for _, _, path in decoded(L, name, place):
                prev, cur = path[:-1], path[1:]
                entries += int(((cur == n_at) & (prev != n_at) & (prev != c_at)).sum())
            assert entries >= 1, (name, place)


@pytest.mark.parametrize("L", SIZES)
def test_family_c_fails_the_check(L):
    for name in names(L, "C"):
        assert any(t >= 1 for t, _ in speculation(L, name)), (name, speculation(L, name))


def test_spec_level2_model_passes_every_check():
    """The `_spec` level-2 model (family A, non-negative scores): the diagonal plan's lane arithmetic
    (tests/diag_l2_cases.py lane_run) fails no check on the control and reproduces the oracle, so the
    level-2 GPU tests may assert that no row was handed over; the relabelled copies' level-2 scores
    are the control's."""
    from tests.chain_place_cases import SPEC_PLACEMENTS, spec_model, spec_seqs
    from tests.diag_l2_cases import lane_run
    from tests.helpers import relabel_chain_hmm

    hmm, rows = spec_model(), spec_seqs()
    assert min(float(hmm.trans_probs.min()), float(hmm.emissions.min()), float(hmm.start_probabilities.min())) >= 0
    refs = oracle.viterbi_spec_batch(hmm, 2, rows)
    for q, seq in enumerate(rows):
        got, fails = lane_run(hmm, seq)
        assert fails == 0 and bit_equal(got, refs[q]), (q, fails)
        assert chain_speculation(hmm, seq)[0] == -1, q
    for place in SPEC_PLACEMENTS:
        hmm2, new = relabel_chain_hmm(hmm, *place)
        refs2 = oracle.viterbi_spec_batch(hmm2, 2, rows)
        assert all(bit_equal(refs2[q][new], refs[q]) for q in range(len(rows))), place
    assert np.isfinite(refs).any()


@pytest.mark.parametrize("L", SIZES)
def test_family_e_dead_row(L):
    """The dead row's score is +inf after the first observation; as a start state it is finite at
    the first."""
    for name in names(L, "E"):
        case = CASES[L][name]
        for place in placements(L):
            _, new, _ = placed(case, place)
            for (s, _, _), seq in zip(decoded(L, name, place), seqs(case)):
                if len(seq) > 1 or not case.start:
                    assert s[new[case.dead]] == np.inf, (name, place, len(seq))
                else:
                    assert np.isfinite(s[new[case.dead]]), (name, place)
        assert not case.start or 1 in case.lengths
