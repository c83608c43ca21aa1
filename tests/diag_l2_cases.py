"""The models and batches of tests/test_diag_l2_gpu.py (`_spec` level 2 on the diagonal plan) and a
numpy restatement of what one lane of that kernel computes.

Kept apart from the GPU tests so that tests/test_diag_l2_cases.py can check without a device that the
inputs the GPU tests assert zero fallbacks for meet that condition by construction: a fallback re-runs
a row on another kernel and would hide a wrong row of the kernel under test.

The restatement (lane_run) follows spec_viterbi_amd/csrc/diag_l2.hip term for term, fp32 with every
add rounded on its own.  Per chunk of two observations with symbols s1, s2, a lane holding
x = v_{p-2}, the feeder score F and the sink score c evaluates, with q = p - 1:

    light   v_p = min(fl(fl(eb_p(s2) + eb_q(s1)) + x),
                      fl(min(fl(eb_p(s2) + ea_q(s1)), fl(ea_p(s2) + X_FF(s1))) + F))
    F'      fl(fl(X_FF(s2) + X_FF(s1)) + F)                         (speculated)
    checks  fl(fl(X_FF(s2) + A_F(s1)) + x) >= F'                    (F, m)
            fl(fl(A_F(s2) + eb_q(s1)) + x) >= F'                    (q, q-1)
            fl(fl(A_F(s2) + ea_q(s1)) + F) >= F'                    (q, F)
            fl(A_F(s1) + x) >= fl(R + fl(emax2 + R) 2^-20), R = fl(X_FF(s1) + F)     (margin)
    S       min(fl(fl(X_SS(s2) + X_SS(s1)) + c), fl(fl(X_SS(s2) + A_S(s1)) + x),
                fl(fl(A_S(s2) + eb_q(s1)) + x), fl(fl(A_S(s2) + ea_q(s1)) + F)) over all lanes

Positions are those of the MSV shape tests.helpers.random_chain_hmm writes: N = state 0 is the feeder
F, M_1 .. M_L are the light positions 0 .. L - 1, C = state L + 1 is the sink S.
"""
from collections import namedtuple

import numpy as np

from tests.helpers import random_chain_hmm, random_seqs

CHUNKS_PER_BLOCK = 32  # diag_l2.hip kLB: a block consumes one ring group of 64 table columns

f32 = np.float32
INF = f32(np.inf)


def inf_feeder(hmm):
    """M -> N at probability 0: the terms exist (the planner needs them) with weight +inf, so A_F = +inf
    and every F check and the margin check pass whatever the scores are."""
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    probs = hmm.trans_probs.copy()
    probs[(cols == 0) & (rows != 0)] = INF
    hmm.trans_probs = probs
    return hmm


def free_feeder(hmm):
    """M -> N free (score 0): the feeder takes its light term, rows fail the check."""
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    probs = hmm.trans_probs.copy()
    probs[(cols == 0) & (rows != 0)] = f32(0.0)
    hmm.trans_probs = probs
    return hmm


def lens_for_chunks(counts):
    """Both tail parities around each chunk count: 2 c + 1 observations (no tail) and 2 c + 2."""
    return [2 * c + 1 + t for c in counts for t in (0, 1)]


Case = namedtuple("Case", "build seqs")


def _case(build, S, lengths, seed):
    return Case(build, lambda: random_seqs(S, lengths, seed=seed))


B = CHUNKS_PER_BLOCK
NP100 = 128  # positions of the L = 100 model's two ranges
# 0, 0, 1, 1, 2, B - 1, B, B + 1, 2 B, 2 B + 1 and 5 B + 1 chunks (every ring group through one full
# turn), one row past 2 NP chunks (every lane wraps through position 0 or 1 four times)
LENGTH_COUNTS = [0, 1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 5 * B + 1, 2 * NP100 + 3]
RANGE_SIZES = [1, 2, 63, 64, 65, 128, 129]
FILL_ROWS = [1, 3, 4, 5, 9]
EDGE_VARIANTS = {
    "ties": dict(ties=True),
    "inf_edges": dict(inf_edges=0.2, zero_emis=0.1),
    "gap": dict(gap=70),
    "start": dict(start=(0, 5)),
}

# every small input the GPU tests assert fallback_rows() == 0 for
NO_FALLBACK_CASES = {"lengths": _case(lambda: inf_feeder(random_chain_hmm(100, S=8, seed=41)), 8, lens_for_chunks(LENGTH_COUNTS), 41)}
for _L in RANGE_SIZES:
    NO_FALLBACK_CASES[f"range{_L}"] = _case(lambda L=_L: inf_feeder(random_chain_hmm(L, S=8, seed=50 + L)), 8,
                                           [1, 4, 67, 2 * B + 2 * _L + 6], 50 + _L)
for _n in FILL_ROWS:
    NO_FALLBACK_CASES[f"fill{_n}"] = _case(lambda: inf_feeder(random_chain_hmm(100, S=8, seed=41)), 8,
                                          [3 + 37 * ((5 * i) % 9) + i for i in range(_n)], 60 + _n)
for _k, _kw in EDGE_VARIANTS.items():
    NO_FALLBACK_CASES[f"edge_{_k}"] = _case(lambda kw=_kw: inf_feeder(random_chain_hmm(150, S=8, seed=70, **kw)), 8,
                                           [1, 2, 3, 64, 131, 2 * B + 2 * 192 + 5], 70)

# the models of test_spec2_pipe_fallback_rows_match_oracle: rows do fall back
FALLBACK_CASES = {
    f"free{n}_{seed}": Case(lambda n=n, seed=seed: free_feeder(random_chain_hmm(n, S=8, seed=seed)),
                            lambda seed=seed: random_seqs(8, [700, 1, 2, 40, 333, 64], seed=seed))
    for n in (300, 1300) for seed in range(3)
}


def chain_tables(hmm):
    """The diagonal plan's view of a random_chain_hmm model, +inf where a term does not exist:
    ea[S, NP], eb[S, NP] (NP = 64 x ranges, +inf dummies past position L - 1), the constants
    A_F, A_S, X_FF, X_SS [S] and emax2 (the largest finite ea)."""
    n, S = int(hmm.states_num), int(hmm.emit_num)
    L = n - 2
    C = n - 1
    NP = (L + 63) // 64 * 64
    em = np.asarray(hmm.emissions, f32).reshape(S, n)
    w = {}
    for a, b, p in zip(hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64), np.asarray(hmm.trans_probs, f32)):
        w.setdefault((int(a), int(b)), f32(p))  # duplicates: the first one wins
    get = lambda a, b: w.get((a, b), INF)
    aw = np.array([get(0, j) for j in range(1, L + 1)], f32)
    bw = np.array([INF] + [get(j - 1, j) for j in range(2, L + 1)], f32)
    wf = {get(j, 0).tobytes() for j in range(1, L + 1)}
    ws = {get(j, C).tobytes() for j in range(1, L + 1)}
    assert len(wf) == 1 and len(ws) == 1, "M -> N and M -> C carry one shared weight each"
    assert (C, 0) not in w and (0, C) not in w and not any((C, j) in w for j in range(1, L + 1)), "not the MSV shape"
    ea = np.full((S, NP), INF, f32)
    eb = np.full((S, NP), INF, f32)
    ea[:, :L] = em[:, 1:L + 1] + aw[None, :]
    eb[:, :L] = em[:, 1:L + 1] + bw[None, :]
    k = dict(A_F=em[:, 0] + get(1, 0), A_S=em[:, C] + get(1, C), X_FF=em[:, 0] + get(0, 0), X_SS=em[:, C] + get(C, C))
    fin = ea[np.isfinite(ea)]
    emax2 = f32(fin.max()) if fin.size else f32(0.0)
    return ea, eb, k, emax2, L, NP


def lane_run(hmm, seq):
    """(final scores [n] float32, failing checks) of one sequence at `_spec` level 2, computed as
    the kernel's lanes do: position p's chunk from x = v_{p-2} alone.  The scores are the level-2
    result only if no check failed.  The odd last observation is the plain step (no speculation)."""
    ea, eb, k, emax2, L, NP = chain_tables(hmm)
    n, S = int(hmm.states_num), int(hmm.emit_num)
    seq = np.asarray(seq, np.int64)
    em = np.asarray(hmm.emissions, f32).reshape(S, n)
    start = np.full(n, INF, f32)
    start[np.asarray(hmm.start_probabilities_cols, np.int64)] = np.asarray(hmm.start_probabilities, f32)
    v0 = (em[seq[0]] + start).astype(f32)
    v = np.full(NP, INF, f32)
    v[:L] = v0[1:L + 1]
    F, c = f32(v0[0]), f32(v0[n - 1])
    fails = 0
    nch = (len(seq) - 1) // 2
    with np.errstate(invalid="ignore"):
        for ch in range(1, nch + 1):
            s1, s2 = seq[2 * ch - 1], seq[2 * ch]
            x = np.roll(v, 2)                                         # x[p] = v[(p - 2) mod NP]
            ea1, eb1 = np.roll(ea[s1], 1), np.roll(eb[s1], 1)         # column q = p - 1
            cb = (eb[s2] + eb1).astype(f32)
            fa = np.minimum((eb[s2] + ea1).astype(f32), (ea[s2] + k["X_FF"][s1]).astype(f32))
            vn = np.minimum((cb + x).astype(f32), (fa + F).astype(f32))
            Fn = f32(f32(k["X_FF"][s2] + k["X_FF"][s1]) + F)
            fm = (f32(k["X_FF"][s2] + k["A_F"][s1]) + x).astype(f32)
            qb = ((k["A_F"][s2] + eb1).astype(f32) + x).astype(f32)
            qa = ((k["A_F"][s2] + ea1).astype(f32) + F).astype(f32)
            fails += int(np.sum(np.minimum(fm, np.minimum(qb, qa)) < Fn))
            R = f32(k["X_FF"][s1] + F)
            thr = f32(R + f32(f32(emax2 + R) * f32(2.0 ** -20)))
            fails += int(np.sum((k["A_F"][s1] + x).astype(f32) < thr))
            ss = f32(f32(k["X_SS"][s2] + k["X_SS"][s1]) + c)
            sm = (f32(k["X_SS"][s2] + k["A_S"][s1]) + x).astype(f32)
            sb = ((k["A_S"][s2] + eb1).astype(f32) + x).astype(f32)
            sa = ((k["A_S"][s2] + ea1).astype(f32) + F).astype(f32)
            c = f32(min(ss, np.min(np.minimum(sm, np.minimum(sb, sa)))))
            v, F = vn, Fn
        if (len(seq) - 1) % 2:  # the tail: one plain step
            o = seq[-1]
            x1 = np.roll(v, 1)
            vn = np.minimum((eb[o] + x1).astype(f32), (ea[o] + F).astype(f32))
            mu = np.min(v)
            Fn = f32(min(f32(k["X_FF"][o] + F), f32(k["A_F"][o] + mu)))
            c = f32(min(f32(k["X_SS"][o] + c), f32(k["A_S"][o] + mu)))
            v, F = vn, Fn
    out = np.empty(n, f32)
    out[0], out[1:L + 1], out[n - 1] = F, v[:L], c
    return out, fails
