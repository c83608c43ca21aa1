"""The inputs of tests/test_diag_l2_gpu.py, checked without a device (tests/diag_l2_cases.py).

The GPU tests of `_spec` level 2 on the diagonal plan assert that no row falls back: a row that
fails a speculation check is re-run by another kernel, which would hide a wrong row.  Whether a row
fails is a property of the model and the sequence, so it is established here with a numpy
restatement of the lane arithmetic (the recurrence, the three F checks and the margin check, fp32,
every add rounded on its own), which is itself held to the oracle bit for bit."""
import numpy as np
import pytest

from oracle import oracle
from tests.diag_l2_cases import (CHUNKS_PER_BLOCK, FALLBACK_CASES, LENGTH_COUNTS, NO_FALLBACK_CASES, NP100, chain_tables,
                                 lane_run, lens_for_chunks)
from tests.helpers import bit_equal, first_mismatch


@pytest.mark.parametrize("name", list(NO_FALLBACK_CASES))
def test_lane_arithmetic_matches_oracle_and_no_check_fails(name):
    """Every small input the GPU file asserts zero flags for: the lane arithmetic reproduces
    oracle.viterbi_spec(level 2) bit for bit and no check fails on any chunk of any row."""
    case = NO_FALLBACK_CASES[name]
    hmm, seqs = case.build(), case.seqs()
    refs = oracle.viterbi_spec_batch(hmm, 2, seqs)
    finite = 0
    for q, seq in enumerate(seqs):
        got, fails = lane_run(hmm, seq)
        assert fails == 0, (name, q, len(seq), fails)
        assert bit_equal(got, refs[q]), (name, q, len(seq), first_mismatch(got, refs[q]))
        finite += int(np.isfinite(refs[q]).sum())
    assert finite > 0, "a batch of +inf rows would pass vacuously"


@pytest.mark.parametrize("name", list(FALLBACK_CASES))
def test_free_feeder_models_fail_a_check(name):
    """The models whose feeder takes its light term (M -> N free): at least one check fails, so
    the GPU test that expects fallbacks there does not depend on the kernel under test."""
    case = FALLBACK_CASES[name]
    hmm, seqs = case.build(), case.seqs()
    assert sum(lane_run(hmm, seq)[1] for seq in seqs) > 0


def test_length_rows_cover_the_block_boundaries():
    """The chunk counts of the lengths case around the kernel's block length, both tail parities,
    and one row long enough for every lane to wrap past the last position more than twice."""
    B = CHUNKS_PER_BLOCK
    lens = lens_for_chunks(LENGTH_COUNTS)
    counts = [(n - 1) // 2 for n in lens]
    for c in (0, 1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 5 * B + 1):
        assert counts.count(c) == 2, c
        assert {(n - 1) % 2 for n in lens if (n - 1) // 2 == c} == {0, 1}
    assert lens[:5] == [1, 2, 3, 4, 5]
    assert max(counts) > 2 * NP100
    hmm = NO_FALLBACK_CASES["lengths"].build()
    assert chain_tables(hmm)[5] == NP100 and int(hmm.emit_num) == 8
