"""CPU: the dense `_spec` products and their run restated in numpy against the oracle, bit for bit.

tests/helpers.py spec_products_numpy / spec_run_numpy are written from the definition in
oracle/viterbi_oracle.h with dense arrays only; oracle/viterbi_oracle.c walks CSR term lists.  Where
the two agree on every bit, tests/test_spec_dense_gpu.py has a reference that two independent
implementations stand behind.  The cases of that file (tests/spec_dense_cases.py) are checked here
too, without a device: each batch covers the keys it claims to, the products fit the memory the
cases are allowed, and the oracle's answer is finite for at least half of the rows.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import spec_dense_cases as cases
from tests.helpers import (bit_equal, covered_keys, first_mismatch, key_cover_seqs, random_hmm, random_seqs, regular_hmm,
                           spec_chunk_keys, spec_products_numpy, spec_run_numpy)

MODELS = {f"random_n{n}_S{S}": (lambda n=n, S=S: random_hmm(n, S=S, out_degree=3, dense_rows=(0, n - 1), zero_emis=0.1,
                                                            seed=7 * n + S), (1, 2, 3, 4))
          for n in (1, 5, 33) for S in (1, 2, 3)}
MODELS["random_n5_S33"] = (lambda: random_hmm(5, S=33, out_degree=2, dense_rows=(4,), seed=33), (2,))
# unreachable states (all-+inf product rows) and +inf emissions, with exact ties
MODELS["regular_unreachable_inf"] = (lambda: regular_hmm(40, S=3, indeg=(1, 2, 3), heavy=(9,), heavy_terms=0.5,
                                                         self_loops=True, ties=True, unreachable=6,
                                                         inf_emis=((9, 0), (9, 2), (20, 1)), zero_emis=0.1, seed=5),
                                     (1, 2, 3))
MODELS["duplicates"] = (lambda: cases.duplicate_hmm(17, 3, 9, copies=20), (1, 2, 3))
MODELS["negative"] = (lambda: cases.neg_hmm(21, 2, 4), (2, 3))

MODEL_LEVELS = [(name, level) for name, (_, levels) in MODELS.items() for level in levels]


@pytest.mark.parametrize("name,level", MODEL_LEVELS)
def test_numpy_products_and_run_equal_the_oracle(name, level):
    hmm = MODELS[name][0]()
    n, S = int(hmm.states_num), int(hmm.emit_num)
    mine = spec_products_numpy(hmm, level)
    ref = oracle.spec_products(hmm, level)
    assert mine.shape == ref.shape == (S ** level, n, n) and mine.dtype == np.float32
    assert bit_equal(mine, ref), first_mismatch(mine, ref)
    assert np.isfinite(ref).any()
    # a key cover (every product is used) with every tail length, and short rows
    seqs = key_cover_seqs(S, level, [r % level for r in range(2 * level)], seed=level) + \
        random_seqs(S, range(1, 2 * level + 3), seed=level + 1)
    assert np.array_equal(covered_keys(seqs, S, level), np.arange(S ** level))
    batch = oracle.viterbi_spec_batch(hmm, level, seqs)
    for q, seq in enumerate(seqs):
        got = spec_run_numpy(hmm, level, seq, mine)
        one = oracle.viterbi_spec(hmm, level, seq)
        assert bit_equal(got, one), (q, len(seq), first_mismatch(got, one))
        assert bit_equal(got, batch[q]), (q, len(seq), first_mismatch(got, batch[q]))


def test_duplicate_model_first_tuple_wins():
    """The duplicate model is not indifferent to the rule: keeping the last tuple, or the smaller
    one, gives other level-1 products."""
    hmm = cases.duplicate_hmm(17, 3, 9, copies=20)
    ref = oracle.spec_products(hmm, 1)
    last = cases.duplicate_hmm(17, 3, 9, copies=20)
    for a in ("trans_rows", "trans_cols", "trans_probs"):
        setattr(last, a, getattr(last, a)[::-1].copy())
    assert not bit_equal(spec_products_numpy(last, 1), ref)
    assert bit_equal(spec_products_numpy(hmm, 1), ref)


@pytest.mark.parametrize("S,level", [(1, 1), (1, 3), (2, 1), (2, 5), (3, 3), (3, 4), (4, 4), (33, 2), (65, 2), (33, 3)])
def test_key_cover_seqs_covers_every_key(S, level):
    tails = [r % level for r in range(max(2 * level, S ** level // 96))]
    seqs = key_cover_seqs(S, level, tails, seed=S + level)
    assert len(seqs) == len(tails)
    assert np.array_equal(covered_keys(seqs, S, level), np.arange(S ** level))
    used = np.concatenate([spec_chunk_keys(s, S, level) for s in seqs])
    assert used.size == max(S ** level, len(tails))  # each key once (more rows than keys: repeats)
    for s, t in zip(seqs, tails):
        assert s.dtype == np.uint64 and s.max() < S
        assert (len(s) - 1) % level == t and (len(s) - 1) // level >= 1
    if S ** level >= 4 * len(tails):
        assert len({len(s) for s in seqs}) > 1  # ragged
    again = key_cover_seqs(S, level, tails, seed=S + level)
    assert all(np.array_equal(a, b) for a, b in zip(seqs, again))
    # the keys follow the base-S rule, first symbol most significant
    s = seqs[0]
    assert spec_chunk_keys(s, S, level)[0] == sum(int(o) * S ** (level - 1 - d) for d, o in enumerate(s[1:1 + level]))


def finite_rows(ref):
    return int(np.isfinite(ref).any(axis=1).sum())


@pytest.mark.parametrize("name", list(cases.CASES))
def test_dense_case_covers_its_keys_and_is_not_vacuous(name):
    hmm, level, kernel, seqs, cover = cases.build(name)
    n, S = int(hmm.states_num), int(hmm.emit_num)
    # device products and the oracle's copy (its level and the one below) stay within 256 MB each
    assert cases.spec_bytes(n, S, level) <= cases.MAX_PRODUCT_BYTES
    assert (S ** level + S ** (level - 1)) * n * n * 4 <= cases.MAX_PRODUCT_BYTES
    assert all(len(s) >= 1 and int(s.max()) < S for s in seqs)
    keys = covered_keys(seqs, S, level)
    if cover:
        assert np.array_equal(keys, np.arange(S ** level))
        nch = [(len(s) - 1) // level for s in seqs]
        assert {(len(s) - 1) % level for s in seqs} == set(range(level))
        assert 0 in nch and 1 in nch and 2 in nch
        assert {c & 1 for c in nch if c >= cases.LONG_CHUNKS} == {0, 1}
    else:
        assert len(seqs) == cases.GRID_ROWS and keys.size > 20000
    ref = oracle.viterbi_spec_batch(hmm, level, seqs)
    assert 2 * finite_rows(ref) >= len(seqs), (finite_rows(ref), len(seqs))


def test_cases_name_every_edge():
    """The shapes the dense-path kernels branch on all have a case."""
    built = {name: c.build() for name, c in cases.CASES.items() if not name.startswith(("chain_", "grid_"))}
    at = {(c.level, int(built[name].emit_num), int(built[name].states_num)) for name, c in cases.CASES.items()
          if name in built}
    for n in (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 260, 511, 513):
        assert (3, 3, n) in at
    for S in (1, 2, 31, 32, 33, 64, 65):
        assert (2, S, 33) in at
    assert {(3, 33, 20), (4, 3, 65), (4, 3, 257), (4, 4, 130), (5, 2, 257)} <= at
    assert {f"chain_{k}" for k in cases.KERNELS} <= set(cases.CASES)
