"""The models and batches of tests/test_spec_dense_gpu.py (the dense `_spec` product path).

Kept apart from the GPU tests so that tests/test_spec_products.py can check, without a device, that
every batch covers the S^level keys it claims to, that the products stay within the memory the
cases are allowed, and that the oracle's answer is not mostly +inf (a vacuous pass).  A case:
id -> Case(model builder, level, kernel preference, batch builder).
"""
from collections import namedtuple

import numpy as np

from tests.helpers import key_cover_seqs, random_chain_hmm, random_hmm, random_seqs, regular_hmm

Case = namedtuple("Case", "build level kernel seqs cover")

MAX_PRODUCT_BYTES = 256 << 20  # device products and the oracle's copy, each
LONG_CHUNKS = 40               # the two long rows run 40 and 41 chunks: both halves of the ping-pong buffer
COVER_CHUNKS = 96              # a key-cover row runs about this many chunks at the most

# kernel preferences by name (spec_viterbi_amd._lib.SVH_KERNEL_*); "auto" is the default
KERNELS = ("auto", "diag", "pipe", "pipe_wide", "chain", "fused")


def spec_bytes(n, S, level):
    """What svh_model_info reports for dense products: S^level matrices of n rows padded to four columns."""
    return S ** level * n * ((n + 3) & ~3) * 4


def one_chunk_seqs(S, level, seed):
    """For every key a row of one observation and that key's chunk, no tail: the row's result is the
    product applied to the first step's vector, so a wrong product row shows without having to lie
    on a later best path."""
    rng = np.random.default_rng(seed)
    keys = np.arange(S ** level, dtype=np.int64)
    digits = (keys[:, None] // (S ** np.arange(level - 1, -1, -1, dtype=np.int64))[None, :]) % S
    rows = np.concatenate([rng.integers(0, S, size=(keys.size, 1)), digits], axis=1).astype(np.uint64)
    return [np.ascontiguousarray(r) for r in rows]


def default_batch(S, level, seed, extra=()):
    """The key cover (every key inside ragged rows, tails of 0 .. level - 1 observations), every key
    once more as the only chunk of a row, rows of 1 .. 2 * level + 2 observations (no chunk, one
    chunk, two chunks, every tail), two long rows whose chunk counts differ in parity (40 chunks
    and a full tail, 41 chunks and none) and rows of the lengths in `extra`."""
    nk = S ** level
    rows = max(2 * level, -(-nk // COVER_CHUNKS))
    seqs = key_cover_seqs(S, level, [r % level for r in range(rows)], seed)
    lens = list(range(1, 2 * level + 3)) + [1 + LONG_CHUNKS * level + level - 1, 1 + (LONG_CHUNKS + 1) * level]
    return seqs + one_chunk_seqs(S, level, seed + 2) + random_seqs(S, lens + list(extra), seed=seed + 1)


def neg_hmm(n, S, seed):
    """tests/test_spec_gpu.py _neg_hmm at a chosen size: a random model with some negative scores
    (p > 1 in the reference's -log2 p terms)."""
    hmm = random_hmm(n, S=S, out_degree=3, dense_rows=(0, 7), seed=seed, zero_emis=0.05)
    rng = np.random.default_rng(seed)
    tp = hmm.trans_probs.copy()
    flip = rng.random(tp.size) < 0.2
    tp[flip & np.isfinite(tp)] *= -0.5
    hmm.trans_probs = tp
    em = hmm.emissions.copy()
    em[(rng.random(em.shape) < 0.1) & np.isfinite(em)] *= -1.0
    hmm.emissions = em
    return hmm


def duplicate_hmm(n, S, seed, copies=60):
    """A random model with `copies` of its transitions stored again further down the list under
    another weight, and its first start state again under another weight (as
    test_gpu_parity.test_duplicate_transitions_first_wins): the first tuple of a pair wins.  Half
    of the copies weigh less than the original, so a last-wins or a min-wins build shows."""
    from spec_viterbi_amd import HMM

    base = random_hmm(n, S=S, out_degree=3, dense_rows=(0, n - 1), seed=seed)
    rng = np.random.default_rng(seed + 1)
    pick = rng.choice(base.trans_rows.size, size=copies, replace=False)
    other = (base.trans_probs[pick] * rng.choice(np.array([0.25, 3.0], np.float32), size=copies)).astype(np.float32)
    return HMM(states_num=n, emit_num=S, trans_num=base.trans_rows.size + copies,
               trans_rows=np.append(base.trans_rows, base.trans_rows[pick]),
               trans_cols=np.append(base.trans_cols, base.trans_cols[pick]),
               trans_probs=np.append(base.trans_probs, other), emissions=base.emissions,
               start_probabilities_cols=np.append(base.start_probabilities_cols, base.start_probabilities_cols[0]),
               start_probabilities=np.append(base.start_probabilities, np.float32(0.125)))


def inf_rows_hmm(n, S, seed):
    """Exact ties, twelve states no term leads into (their product rows are all +inf) and +inf
    emissions: each heavy row for one or two of the three symbols, state 0 for one."""
    return regular_hmm(n, S=S, indeg=(2, 3), heavy=(5, n - 2), heavy_terms=0.5, heavy_heavy=1, self_loops=True, ties=True,
                       unreachable=12, inf_emis=((5, 0), (5, 2), (n - 2, 1), (0, 1)), zero_emis=0.05, seed=seed)


CASES = {}


def case(name, build, level, kernel="auto", seqs=None, cover=True, seed=None, extra=()):
    assert name not in CASES and kernel in KERNELS
    seed = sum(map(ord, name)) if seed is None else seed
    if seqs is None:
        def seqs(hmm, level=level, seed=seed, extra=extra):
            return default_batch(int(hmm.emit_num), level, seed, extra)
    CASES[name] = Case(build, level, kernel, seqs, cover)


# ---- row and column tiles: one lane, one wave, 32 rows per workgroup of the chunk kernel, the
#      padding columns [n, pstride), one / two / three 256-column tiles of the extend kernel ---------
TILE_N = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 260, 511, 513)
for n in TILE_N:
    case(f"tile_n{n}", lambda n=n: random_hmm(n, S=3, out_degree=3, dense_rows=(0, n - 1), seed=n), 3)

# ---- symbol chunks of the extend kernel (32 symbols per workgroup); level 2 by the dense flag ------
SYMBOLS_L2 = (1, 2, 31, 32, 33, 64, 65)
for S in SYMBOLS_L2:
    case(f"sym_l2_S{S}", lambda S=S: random_hmm(33, S=S, out_degree=3, dense_rows=(0, 32), seed=S), 2)
# kprev = 1089 keys x nsc = 2 symbol chunks in blockIdx.z
case("sym_l3_S33", lambda: random_hmm(20, S=33, out_degree=3, dense_rows=(0, 19), seed=333), 3)

# ---- deeper levels ---------------------------------------------------------------------------------
for level, S, n in [(4, 3, 65), (4, 3, 257), (4, 4, 130), (5, 2, 257)]:
    case(f"deep_l{level}_S{S}_n{n}",
         lambda S=S, n=n: random_hmm(n, S=S, out_degree=3, dense_rows=(0, n - 1), seed=10 * n + S), level)

# ---- numeric content, level 3 on 260 states --------------------------------------------------------
case("num_zero_emis", lambda: random_hmm(260, S=3, out_degree=3, dense_rows=(0, 259), zero_emis=0.2, seed=71), 3)
case("num_inf_rows", lambda: inf_rows_hmm(260, 3, 72), 3)
case("num_negative", lambda: neg_hmm(260, 3, 73), 3)
case("num_duplicates", lambda: duplicate_hmm(260, 3, 74), 3)
# start vectors with one, two and n finite entries: one start state exposes single product columns
for level in (2, 3):
    for nstart in (1, 2, 257):
        case(f"start{nstart}_l{level}",
             lambda nstart=nstart: random_hmm(257, S=3, out_degree=3, dense_rows=(0, 256), nstart=nstart, seed=80 + nstart),
             level)

# ---- chain-shaped models: the chunks' tail under every step kernel; rows of 256 .. 260 observations
#      end their 85 or 86 chunks at observation 256 or 259 with every tail length -------------------
for kern in KERNELS:
    case(f"chain_{kern}", lambda: random_chain_hmm(700, S=3, seed=91), 3, kernel=kern, seed=91,
         extra=(256, 257, 258, 259, 260))

# ---- the largest grid the extend kernel accepts: S = 127 at level 3 is kprev = 16129 keys x nsc = 4
#      symbol chunks = 64516 <= 65535 planes; a 300-row sample of a cover of its 2048383 keys --------
GRID_S, GRID_N, GRID_ROWS = 127, 3, 300


def grid_limit_sample(hmm):
    rows = -(-GRID_S ** 3 // COVER_CHUNKS)
    cover = key_cover_seqs(GRID_S, 3, [r % 3 for r in range(rows)], seed=127)
    return cover[::rows // GRID_ROWS][:GRID_ROWS]


case("grid_limit_S127", lambda: random_hmm(GRID_N, S=GRID_S, out_degree=3, dense_rows=(0, 2), seed=127), 3,
     seqs=grid_limit_sample, cover=False)


def build(name):
    """(model, level, kernel name, sequences, whether the batch covers every key) of a case."""
    c = CASES[name]
    hmm = c.build()
    return hmm, c.level, c.kernel, c.seqs(hmm), c.cover
