"""The models and batches of tests/test_chain_place_gpu.py: chain-shaped models whose feeder row N
and sink row C sit at any state index.

Every other chain model of the suite has N = state 0, the light rows M_1 .. M_L = states 1 .. L and
C = state L + 1, so the kernels' scatter through lrow / rowF / rowS, the (value, row) argmin of the
best state and every tie rule of the decoded paths that compares a heavy row's index with a light
row's (pflags bit 2, f_self, min(hcol, js)) see one constant outcome there.  The models here are
tests.helpers.random_chain_hmm models moved by tests.helpers.relabel_chain_hmm; the families:

    A  ties=True, n_from_m=False: integer scores (exact ties everywhere), F has no light term, so no
       row can fail the speculation check
    B  ties=True, then N -> N = 0.0f and every M -> N = 3.0f: F's light term ties with its self term
       without ever beating it (the check is strict), so with N above the light rows the oracle's
       backpointer of N is a light row
    C  default weights with every M -> N = 0.0f: rows fail the check and are re-run
    D  A plus N -> C at 3.0f (the sink's X_SF term)
    E  A with one light row dead: N -> M_j and M_{j-1} -> M_j deleted (its pflags are 0, ties_heavy is
       false); "start": the dead row is a start state

Kept apart from the GPU tests so that tests/test_chain_place_cases.py can establish without a device
what the GPU tests rely on: that the relabelled models' tie outcomes differ from the control's, that
families A, B and D cannot fall back and that family C does.
"""
from collections import namedtuple

import numpy as np

from tests.helpers import random_chain_hmm, random_seqs, relabel_chain_hmm

S = 12
f32 = np.float32


def placements(L):
    """(n_at, c_at): the control, N and C swapped, C first and N second (F still wins every tie),
    both last, both interior at a wave boundary (lrow shifts by 2 from position 64 on), only C moved."""
    return [(0, L + 1), (L + 1, 0), (1, 0), (L + 1, L), (64, 65), (0, 130)]


def _set_weights(hmm, m_to_n=None, n_to_n=None):
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    probs = hmm.trans_probs.copy()
    if m_to_n is not None:
        probs[(cols == 0) & (rows != 0)] = f32(m_to_n)
    if n_to_n is not None:
        probs[(cols == 0) & (rows == 0)] = f32(n_to_n)
    hmm.trans_probs = probs
    return hmm


def family_a(L, seed):
    return random_chain_hmm(L, S=S, seed=seed, ties=True, n_from_m=False)


def family_b(L, seed):
    return _set_weights(random_chain_hmm(L, S=S, seed=seed, ties=True), m_to_n=3.0, n_to_n=0.0)


def family_c(L, seed):
    return _set_weights(random_chain_hmm(L, S=S, seed=seed), m_to_n=0.0)


def family_d(L, seed):
    hmm = family_a(L, seed)
    hmm.trans_rows = np.append(hmm.trans_rows, np.uint64(0))
    hmm.trans_cols = np.append(hmm.trans_cols, np.uint64(L + 1))
    hmm.trans_probs = np.append(hmm.trans_probs, f32(3.0))
    hmm.trans_num = int(hmm.trans_probs.size)
    return hmm


def family_e(L, seed, dead, start=False):
    hmm = random_chain_hmm(L, S=S, seed=seed, ties=True, n_from_m=False, start=(0, dead) if start else (0,))
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    keep = ~((cols == dead) & ((rows == 0) | (rows == dead - 1)))
    assert keep.sum() == hmm.trans_num - 2
    hmm.trans_rows, hmm.trans_cols, hmm.trans_probs = hmm.trans_rows[keep], hmm.trans_cols[keep], hmm.trans_probs[keep]
    hmm.trans_num = int(keep.sum())
    return hmm


# family: "A" .. "E"; dead: family E's dead light row (control index) or None; start: it is a start state
Case = namedtuple("Case", "family L seed lengths dead start")


def _case(family, L, seed, lengths, dead=None, start=False):
    return Case(family, L, seed, tuple(lengths), dead, start)


def build(case):
    """The control model (N = 0, C = L + 1) of a case."""
    if case.family == "E":
        return family_e(case.L, case.seed, case.dead, case.start)
    return {"A": family_a, "B": family_b, "C": family_c, "D": family_d}[case.family](case.L, case.seed)


def seqs(case):
    return random_seqs(S, case.lengths, seed=case.seed)


def placed(case, place):
    """(relabelled model, new[old state], control model)."""
    hmm = build(case)
    hmm2, new = relabel_chain_hmm(hmm, *place)
    return hmm2, new, hmm


def feeder_wins_every_tie(case, place):
    """PipePlan::ties_heavy (runtime.cpp make_pipe_plan) restated: every light row takes a term from
    F, and F's state index is below every light row's (pflags bit 2 at every position).  The
    diagonal path variant is planned for these models only."""
    first_light = min(j for j in range(3) if j not in place)
    return case.family != "E" and place[0] < first_light


LENS = (1, 2, 33, 64, 97, 130)       # rows of one batch: at most six, none longer than 300
LENS_B = (33, 64, 97, 130, 300)       # family B: the lengths its input conditions were measured at
LENS_2 = (3, 65, 300)

# L per plan: chain and band 300; the diagonal plan 200 and 130 (two ranges of 128 positions, the
# second almost all dummies); the latency plan 700 (two workgroups); the wide plan 1300 (three blocks)
PLAN_L = {"chain": 300, "band": 300, "diag": 200, "diag130": 130, "pipe": 700, "pipew": 1300}


# Seeds (model and sequences) per model size, chosen so that the oracle alone meets the input
# conditions of tests/test_chain_place_cases.py: families A and B move path entries and best states
# at every placement; every row of a family B case passes the check, at least half of them with a
# tied feeder term, and with N last the oracle's path enters N from a light row.
SEEDS = {  # L: (A, A2, B, B2)
    130: (3, 1, 13, 17),
    200: (0, 3, 1, 16),
    300: (7, 1, 1, 17),
    700: (5, 1, 1, 17),
    1300: (1, 0, 18, 5),
}


def _family_cases(L):
    """The cases of one model size."""
    dead = [j for j in (150, 64) if j < L]
    a, a2, b, b2 = SEEDS[L]
    cases = {
        "A": _case("A", L, a, LENS),
        "A2": _case("A", L, a2, LENS_2),
        "B": _case("B", L, b, LENS_B),
        "B2": _case("B", L, b2, LENS_B),
        "D": _case("D", L, 2, LENS),
    }
    for j in dead:
        cases[f"E{j}"] = _case("E", L, 3, LENS, dead=j)
    cases["Estart"] = _case("E", L, 4, LENS, dead=dead[-1], start=True)
    for seed in range(3):
        cases[f"C{seed}"] = _case("C", L, seed, LENS_B)
    return cases


CASES = {L: _family_cases(L) for L in sorted(set(PLAN_L.values()))}


def names(L, families):
    return [k for k, c in CASES[L].items() if c.family in families]


# `_spec` level 2: family A (every score >= 1: non-negative), tiny products
SPEC_L, SPEC_S = 100, 3
SPEC_PLACEMENTS = [(SPEC_L + 1, 0), (64, 65)]
SPEC_LENS = (2, 3, 64, 301)


def spec_model(seed=5):
    return random_chain_hmm(SPEC_L, S=SPEC_S, seed=seed, ties=True, n_from_m=False)


def spec_seqs(seed=5):
    return random_seqs(SPEC_S, SPEC_LENS, seed=seed)
