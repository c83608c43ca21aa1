"""Shared helpers: golden loading, exact float comparison, synthetic models."""
from __future__ import annotations

import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, f"{name}.json")) as f:
        return json.load(f)


def load_digests():
    """tests/golden/score_digests.json: per-row SHA-256 of the oracle's float32 scores (+ paths)."""
    with open(os.path.join(GOLDEN, "score_digests.json")) as f:
        return json.load(f)


def from_hex(bits):
    return np.array([struct.unpack("<f", bytes.fromhex(b))[0] for b in bits], np.float32)


def bit_equal(a, b) -> bool:
    """Bit-exact fp32 equality, except that -0.0 == +0.0 (min of equal zeros may pick either)."""
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    same = ua == ub
    zeros = (a == 0) & (b == 0)
    return bool(np.all(same | zeros))


def first_mismatch(a, b):
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    bad = np.nonzero(~((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return i, float(a[i]), float(b[i]), int(bad.size)


def random_hmm(n, S=20, out_degree=3, nstart=2, seed=0, dense_rows=(), self_loops=False, zero_emis=0.0):
    """chmm_gen.py-shaped random model (reference chmm_files/chmm_gen.py:1-62), seeded.

    dense_rows: states that every other state also transitions into (heavy rows).
    """
    from spec_viterbi_amd import HMM

    rng = np.random.default_rng(seed)
    nstart = min(nstart, n)

    def probs(k):
        w = rng.integers(1, 100, size=k).astype(np.float64)
        return (w / w.sum()).astype(np.float32)

    src, dst, pr = [], [], []
    for s in range(n):
        targets = rng.choice(n, size=min(out_degree, n), replace=False)
        for d, p in zip(targets, probs(targets.size)):
            src.append(s)
            dst.append(int(d))
            pr.append(p)
        if self_loops:
            src.append(s)
            dst.append(s)
            pr.append(np.float32(0.5))
    for d in dense_rows:
        for s in range(n):
            src.append(s)
            dst.append(d)
            pr.append(np.float32(0.01))
    em = np.stack([probs(S) for _ in range(n)]).T.copy()  # [S][n]
    if zero_emis > 0:
        em[rng.random(em.shape) < zero_emis] = 0.0

    def mod(p):
        p = np.asarray(p, np.float32)
        with np.errstate(divide="ignore"):
            return np.where(p > 0, -np.log2(p), np.inf).astype(np.float32)

    return HMM(states_num=n, emit_num=S, trans_num=len(pr), trans_rows=np.array(src, np.uint64),
               trans_cols=np.array(dst, np.uint64), trans_probs=mod(pr), emissions=mod(em),
               start_probabilities_cols=np.arange(nstart, dtype=np.uint64),
               start_probabilities=mod(probs(nstart)))


def random_seqs(S, lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, S, size=int(L)).astype(np.uint64) for L in lengths]


def random_chain_hmm(L, S=20, seed=0, self_n=True, self_c=True, feed_c=False, c_from_m=True, n_from_m=True,
                     zero_emis=0.0, gap=None, start=(0,), ties=False, inf_edges=0.0, **_):
    """MSV-shaped random model (the shape chmm_files/silent_hmm_to_chmm.py writes): N=0, M_1..M_L,
    C=L+1.  N -> M_j, M_j -> M_{j+1}, M_j -> N and M_j -> C with one shared weight each, N and C
    self loops.  Variants: feed_c adds C -> M_j (light rows fed by two heavy rows); c_from_m /
    n_from_m drop the uniform M -> heavy terms; gap drops M_gap -> M_gap+1 (chain break); ties draws
    every probability from {1/2, 1/4, 1/8} (integer scores: exact ties everywhere); inf_edges sets
    that fraction of the light rows' terms to probability 0 (the term exists, weight +inf)."""
    from spec_viterbi_amd import HMM

    rng = np.random.default_rng(seed)
    n = L + 2
    C = L + 1
    src, dst, pr = [], [], []

    def add(a, b, p, shared=False):
        if ties and not shared:
            p = float(rng.choice([0.5, 0.25, 0.125]))
        if inf_edges > 0 and b not in (0, C) and rng.random() < inf_edges:
            p = 0.0
        src.append(a)
        dst.append(b)
        pr.append(np.float32(p))

    w_n, w_c = rng.uniform(0.01, 0.2), rng.uniform(0.01, 0.2)
    if ties:
        w_n, w_c = float(rng.choice([0.5, 0.25, 0.125])), float(rng.choice([0.5, 0.25, 0.125]))
    for j in range(1, L + 1):
        add(0, j, rng.uniform(0.001, 0.05))
        if feed_c:
            add(C, j, rng.uniform(0.001, 0.05))
        if j < L and j != gap:
            add(j, j + 1, rng.uniform(0.3, 0.9))
        if n_from_m:
            add(j, 0, w_n, shared=True)
        if c_from_m:
            add(j, C, w_c, shared=True)
    if self_n:
        add(0, 0, rng.uniform(0.5, 0.99))
    if self_c:
        add(C, C, rng.uniform(0.5, 0.99))
    em = rng.uniform(0.001, 1.0, size=(S, n)).astype(np.float32)
    if ties:
        em = rng.choice(np.array([0.5, 0.25, 0.125], np.float32), size=(S, n))
    if zero_emis > 0:
        em[rng.random(em.shape) < zero_emis] = 0.0

    def mod(p):
        p = np.asarray(p, np.float32)
        with np.errstate(divide="ignore"):
            return np.where(p > 0, -np.log2(p), np.inf).astype(np.float32)

    st = np.array(start, np.uint64)
    return HMM(states_num=n, emit_num=S, trans_num=len(pr), trans_rows=np.array(src, np.uint64),
               trans_cols=np.array(dst, np.uint64), trans_probs=mod(pr), emissions=mod(em),
               start_probabilities_cols=st, start_probabilities=mod(rng.uniform(0.1, 1.0, size=st.size)))


def relabel_chain_hmm(hmm, n_at, c_at):
    """A random_chain_hmm model (N = 0, M_1..M_L, C = L + 1) with N at state `n_at`, C at `c_at` and
    the light rows at the remaining indices in their original order: (hmm2, new), new[old state] the
    index map.  Only indices move: every weight, the order of the tuples and every float stay."""
    from spec_viterbi_amd import HMM

    n = int(hmm.states_num)
    L = n - 2
    assert 0 <= n_at < n and 0 <= c_at < n and n_at != c_at
    new = np.empty(n, np.int64)
    new[0], new[L + 1] = n_at, c_at
    new[1:L + 1] = [j for j in range(n) if j not in (n_at, c_at)]
    em = np.empty_like(hmm.emissions)
    em[:, new] = hmm.emissions
    hmm2 = HMM(states_num=n, emit_num=int(hmm.emit_num), trans_num=int(hmm.trans_num),
               trans_rows=new[hmm.trans_rows.astype(np.int64)].astype(np.uint64),
               trans_cols=new[hmm.trans_cols.astype(np.int64)].astype(np.uint64), trans_probs=hmm.trans_probs.copy(),
               emissions=em, start_probabilities_cols=new[hmm.start_probabilities_cols.astype(np.int64)].astype(np.uint64),
               start_probabilities=hmm.start_probabilities.copy())
    return hmm2, new


def chain_speculation(hmm, seq):
    """The pipelined plans' speculation check (kernels.h, PipeModel) restated in numpy float32 for an
    unrelabelled random_chain_hmm model (N = 0, C = L + 1; N -> C and dead light rows allowed): the
    exact recurrence observation by observation, every add rounded on its own and associated as the
    oracle's (emission plus weight first, then the score).  Returns (t_first, ties): the first
    observation t >= 1 with fl(fl(E[o_t][N] + w_MN) + min_j v_{t-1}[M_j]) <
    fl(fl(E[o_t][N] + w_NN) + v_{t-1}[N]), or -1; and the number of observations before it (all of
    them if -1) at which the two sides are equal and finite."""
    f32 = np.float32
    n, S = int(hmm.states_num), int(hmm.emit_num)
    L = n - 2
    E = np.asarray(hmm.emissions, f32).reshape(S, n)
    src, dst, w = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64), np.asarray(hmm.trans_probs, f32)
    assert np.unique(dst * n + src).size == src.size, "no duplicate transitions"
    wmn = w[(dst == 0) & (src != 0)]
    assert wmn.size in (0, L) and (wmn.view(np.uint32) == wmn.view(np.uint32)[:1]).all(), "M -> N: one shared weight"
    w_mn = wmn[0] if wmn.size else f32(np.inf)
    wnn = w[(dst == 0) & (src == 0)]
    w_nn = wnn[0] if wnn.size else f32(np.inf)
    start = np.full(n, np.inf, f32)
    start[hmm.start_probabilities_cols.astype(np.int64)] = np.asarray(hmm.start_probabilities, f32)
    v = E[int(seq[0])] + start
    ties = 0
    for t in range(1, len(seq)):
        o = int(seq[t])
        light = f32(f32(E[o][0] + w_mn) + v[1:L + 1].min())
        own = f32(f32(E[o][0] + w_nn) + v[0])
        if light < own:
            return t, ties
        ties += int(light == own and np.isfinite(own))
        nxt = np.full(n, np.inf, f32)
        np.minimum.at(nxt, dst, (E[o][dst] + w) + v[src])  # v'[j] = min_k fl(fl(E[o][j] + T[k][j]) + v[k])
        v = nxt
    return -1, ties


def regular_hmm(n, S=4, indeg=(2,), heavy=(), heavy_terms=1.0, heavy_heavy=0, self_loops=False, zero_emis=0.0,
                ties=False, unreachable=0, start=None, nstart=2, inf_emis=(), seed=0):
    """A random model with a controlled in-degree, so that a test can aim at one fused-kernel family.

    Every light row's in-degree is drawn uniformly from `indeg` ({R}: exactly R; range(1, R + 1): up
    to R); its sources are drawn without replacement over the whole state range (LDS gathers cross
    slots and waves), and for every heavy row three light rows take it as a source.  `heavy` rows
    receive a term from a fraction `heavy_terms` of the light states, each with its own random weight
    (general, not uniform heavy rows), plus terms from their first `heavy_heavy` fellow heavy rows
    and, with `self_loops`, from themselves (the kernels' exception terms).  `unreachable`: that many
    light states (or the given ones) get no incoming term and no start entry; they still are sources.
    `ties` draws every probability from {1/2, 1/4, 1/8}.  `start`: the start states (default: the
    first `nstart` states that are not unreachable).  `inf_emis`: (state, symbol) pairs of
    probability 0 on top of the random fraction `zero_emis`."""
    from spec_viterbi_amd import HMM

    rng = np.random.default_rng(seed)
    heavy = tuple(int(h) for h in heavy)
    is_heavy = np.zeros(n, bool)
    is_heavy[list(heavy)] = True
    light = np.nonzero(~is_heavy)[0]
    if isinstance(unreachable, int):
        unreachable = rng.choice(light, size=unreachable, replace=False) if unreachable else ()
    dead = np.zeros(n, bool)
    dead[list(unreachable)] = True
    assert not (dead & is_heavy).any()
    indeg = np.array(sorted(indeg))
    assert indeg[-1] <= n

    def prob(k):
        if ties:
            return rng.choice(np.array([0.5, 0.25, 0.125], np.float32), size=k)
        return rng.uniform(0.01, 1.0, size=k).astype(np.float32)

    src, dst = [], []
    feeds = {}  # light row -> a heavy row it must take as a source
    live = light[~dead[light]]
    for h in heavy:
        for j in rng.choice(live, size=min(3, live.size), replace=False):
            feeds.setdefault(int(j), h)
    for j in live:
        k = rng.choice(n, size=int(rng.choice(indeg)), replace=False)
        h = feeds.get(int(j))
        if h is not None and k.size and h not in k:
            k[0] = h
        src.append(k)
        dst.append(np.full(k.size, j))
    for x, h in enumerate(heavy):
        cnt = max(1, int(round(heavy_terms * light.size)))
        k = [rng.choice(light, size=cnt, replace=False)]
        others = [o for o in heavy if o != h]
        k.append(np.array([others[(x + d) % len(others)] for d in range(min(heavy_heavy, len(others)))], np.int64))
        if self_loops:
            k.append(np.array([h]))
        k = np.concatenate(k)
        src.append(k)
        dst.append(np.full(k.size, h))
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    dst = np.concatenate(dst) if dst else np.zeros(0, np.int64)
    pr = prob(src.size)
    em = prob(S * n).reshape(S, n)
    if zero_emis > 0:
        em[rng.random(em.shape) < zero_emis] = 0.0
    for j, o in inf_emis:
        em[o, j] = 0.0
    if start is None:
        start = np.nonzero(~dead)[0][:nstart]
    st = np.array(start, np.uint64)
    assert not dead[st.astype(np.int64)].any()

    def mod(p):
        p = np.asarray(p, np.float32)
        with np.errstate(divide="ignore"):
            return np.where(p > 0, -np.log2(p), np.inf).astype(np.float32)

    return HMM(states_num=n, emit_num=S, trans_num=int(pr.size), trans_rows=src.astype(np.uint64),
               trans_cols=dst.astype(np.uint64), trans_probs=mod(pr), emissions=mod(em),
               start_probabilities_cols=st, start_probabilities=mod(prob(st.size)))


def in_degrees(hmm):
    """In-degree of every state over distinct (source, destination) pairs (duplicates count once)."""
    n = int(hmm.states_num)
    pairs = np.unique(hmm.trans_cols.astype(np.int64) * n + hmm.trans_rows.astype(np.int64))
    return np.bincount(pairs // n, minlength=n)


# The fused planner's rules (runtime.cpp make_plan), restated: families (R, HM, XM, uniform heavy
# rows) in the order they are tried, slot counts, workgroup cap and the LDS a geometry needs.
FUSED_FAMILIES = ((2, 2, 2, True), (2, 2, 2, False), (4, 4, 4, False), (8, 4, 4, False), (16, 4, 4, False))
FUSED_SLOTS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)
FUSED_MAX_THREADS = 512
FUSED_MAX_LDS = 160 * 1024
GENERIC_MAX_THREADS = 1024


def fused_lds_bytes(sm, B, vstride):
    ndma = (sm + 3) // 4
    return (3 * vstride + 3 * ndma * B * 4) * 4 + 3 * 4 * 8 + 2 * 16 * 4 + 4096 + 64 + 16


def _uniform_heavy(hmm, heavy, XM):
    """analyse_uniform: every heavy row is one dominant weight over a light source set shared by all
    heavy rows plus at most XM other terms."""
    if not heavy:
        return False
    rows, cols = hmm.trans_rows.astype(np.int64), hmm.trans_cols.astype(np.int64)
    _, first = np.unique(cols * int(hmm.states_num) + rows, return_index=True)
    rows, cols, vals = rows[first], cols[first], hmm.trans_probs[first]
    hset = set(heavy)
    shared = None
    for h in heavy:
        sel = cols == h
        k, w = rows[sel], vals[sel].view(np.uint32)
        lightsrc = np.array([x not in hset for x in k], bool)
        u = np.zeros(0, np.int64)
        if lightsrc.any():
            bits, cnt = np.unique(w[lightsrc], return_counts=True)
            u = np.sort(k[lightsrc & (w == bits[np.argmax(cnt)])])  # first maximum: the lowest weight bits
        if k.size - u.size > XM:
            return False
        if shared is None:
            shared = u
        elif not np.array_equal(u, shared):
            return False
    return True


def expected_plan(hmm, max_threads=0, allow_uniform=True):
    """What svh_model_info must report for this model's step kernel: dict(fused, family, slots,
    threads, light_terms, heavy_rows, heavy_uniform); family -1 / slots 0: the generic kernel."""
    n = int(hmm.states_num)
    deg = in_degrees(hmm)
    cap = min(max_threads, FUSED_MAX_THREADS) if max_threads > 0 else FUSED_MAX_THREADS
    generic = dict(fused=False, family=-1, slots=0, threads=min(GENERIC_MAX_THREADS, (n + 63) // 64 * 64),
                   light_terms=0, heavy_rows=0, heavy_uniform=0)
    for fam, (R, HM, XM, uniform) in enumerate(FUSED_FAMILIES):
        if uniform and not allow_uniform:
            continue
        heavy = [int(j) for j in np.nonzero(deg > R)[0]]
        if len(heavy) > HM:
            continue
        if uniform and not _uniform_heavy(hmm, heavy, XM):
            continue
        for sm in FUSED_SLOTS:
            B = max(64, ((n + sm - 1) // sm + 63) // 64 * 64)
            if B > cap:
                continue
            vstride = (sm * B + 1 + 4 + 3) // 4 * 4
            if fused_lds_bytes(sm, B, vstride) > FUSED_MAX_LDS:
                continue
            return dict(fused=True, family=fam, slots=sm, threads=B, light_terms=R, heavy_rows=len(heavy),
                        heavy_uniform=int(uniform))
        return generic
    return generic


# The dense `_spec` products and their run, restated from the definition in oracle/viterbi_oracle.h
# with dense numpy arrays only (no CSR, no term lists): an implementation independent of both the
# oracle's C and the device kernels.  Every add is one float32 add; +inf stands for "no term", and
# fl(+inf + x) = +inf never wins a minimum, so minimising over every index equals minimising over
# the stored terms (no score is -inf or NaN).
def _dense_model(hmm):
    """(E [S, n], T^T [n, n], start [n]) in float32: T^T[j][k] is the weight of k -> j, the first
    tuple of a duplicate (k, j) wins; absent entries are +inf."""
    n, S = int(hmm.states_num), int(hmm.emit_num)
    E = np.asarray(hmm.emissions, np.float32).reshape(S, n)
    tt = np.full((n, n), np.inf, np.float32)
    dst, src = hmm.trans_cols.astype(np.int64), hmm.trans_rows.astype(np.int64)
    _, first = np.unique(dst * n + src, return_index=True)  # the first occurrence of every (k, j)
    tt[dst[first], src[first]] = np.asarray(hmm.trans_probs, np.float32)[first]
    start = np.full(n, np.inf, np.float32)
    cols = hmm.start_probabilities_cols.astype(np.int64)
    _, first = np.unique(cols, return_index=True)
    start[cols[first]] = np.asarray(hmm.start_probabilities, np.float32)[first]
    return E, tt, start


def _minplus(A, B):
    """C[j][m] = min_p fl(A[j][p] + B[p][m]) in float32 (B may be a vector)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    if B.ndim == 1:
        return (A + B[None, :]).min(axis=1)
    out = np.empty((A.shape[0], B.shape[1]), np.float32)
    for j in range(A.shape[0]):  # row by row: n^2 floats live, not n^3
        out[j] = (A[j][:, None] + B).min(axis=0)
    return out


def spec_products_numpy(hmm, level):
    """Dense level-`level` products [S^level, n, n] float32: M_o[j][k] = fl(E[o][j] + T^T[j][k]),
    H[(k..., i)] = M_i (x) H[(k...)]; keys base S, the first symbol most significant."""
    assert level >= 1
    S = int(hmm.emit_num)
    E, tt, _ = _dense_model(hmm)
    M = E[:, :, None] + tt[None, :, :]
    H = M
    for _ in range(1, level):
        H = np.stack([_minplus(M[i], H[k]) for k in range(H.shape[0]) for i in range(S)])
    return H


def spec_run_numpy(hmm, level, seq, products):
    """Final scores [n] of one sequence at `_spec` level `level` (<= 1: every observation is a tail
    step): v0 = fl(E[s0] + start), one product per `level` observations while that many remain,
    then v' = M_o (x) v per observation."""
    S = int(hmm.emit_num)
    E, tt, start = _dense_model(hmm)
    seq = [int(o) for o in seq]
    v = E[seq[0]] + start
    i = 1
    if level > 1:
        assert products.shape[0] == S ** level
        while len(seq) - i >= level:
            key = 0
            for o in seq[i:i + level]:
                key = key * S + o
            v = _minplus(products[key], v)
            i += level
    for o in seq[i:]:
        v = _minplus(E[o][:, None] + tt, v)
    return v


def spec_chunk_keys(seq, S, level):
    """The product keys the chunks of one sequence use, in order."""
    nch = (len(seq) - 1) // level
    d = np.asarray(seq[1:1 + nch * level], np.int64).reshape(nch, level)
    return d @ (S ** np.arange(level - 1, -1, -1, dtype=np.int64))


def key_cover_seqs(S, level, tail_lens, seed):
    """A ragged batch of len(tail_lens) sequences whose chunks use every one of the S^level keys
    (each once, in a random order, dealt out in random uneven shares of at least one chunk; where
    there are fewer keys than sequences some keys repeat).  Sequence r = a first observation, its
    chunks, and a tail of tail_lens[r] observations (0 .. level - 1)."""
    rng = np.random.default_rng(seed)
    R = len(tail_lens)
    assert R >= 1 and all(0 <= t < max(level, 1) for t in tail_lens)
    nk = S ** level
    keys = rng.permutation(nk)
    if nk < R:
        keys = np.concatenate([keys, rng.integers(0, nk, size=R - nk)])
    cuts = np.sort(rng.choice(np.arange(1, keys.size), size=R - 1, replace=False)) if R > 1 else []
    digits = (keys[:, None] // (S ** np.arange(level - 1, -1, -1, dtype=np.int64))[None, :]) % S
    seqs = []
    for part, tail in zip(np.split(digits, cuts), tail_lens):
        seqs.append(np.concatenate([rng.integers(0, S, size=1), part.ravel(), rng.integers(0, S, size=int(tail))])
                    .astype(np.uint64))
    return seqs


def covered_keys(seqs, S, level):
    """Sorted distinct keys the chunks of a batch use."""
    return np.unique(np.concatenate([spec_chunk_keys(s, S, level) for s in seqs]))
