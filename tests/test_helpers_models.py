"""CPU: the generated models of the fused / generic GPU tests are what their cases ask for.

regular_hmm's in-degree histogram, heavy set, exception terms, unreachable states and ties are
recomputed here from the model's transition arrays, and every case of tests/fused_cases.py is run
through the planner's rules restated in numpy (tests/helpers.py expected_plan): family, slots,
threads and heavy rows must be the ones the case names.  tests/test_fused_gpu.py asserts the same
fields from the device, so a generator or planner change cannot move a GPU case to another kernel
instance unnoticed.
"""
import numpy as np
import pytest

from tests import fused_cases
from tests.helpers import expected_plan, fused_lds_bytes, in_degrees, regular_hmm


def sources(hmm, j):
    return set(int(r) for r, c in zip(hmm.trans_rows, hmm.trans_cols) if int(c) == j)


@pytest.mark.parametrize("R", [2, 4, 8, 16])
def test_light_in_degrees_are_drawn_from_the_set(R):
    exact = regular_hmm(400, indeg=(R,), seed=R)
    assert np.all(in_degrees(exact) == R)
    upto = regular_hmm(400, indeg=range(1, R + 1), seed=R)
    deg = in_degrees(upto)
    assert deg.min() >= 1 and deg.max() == R and set(deg) == set(range(1, R + 1))
    assert hmm_pairs_unique(upto)
    # sources cover the whole state range (gathers cross slots and waves)
    assert upto.trans_rows.min() < 20 and upto.trans_rows.max() >= 380


def hmm_pairs_unique(hmm):
    pairs = hmm.trans_cols.astype(np.int64) * int(hmm.states_num) + hmm.trans_rows.astype(np.int64)
    return np.unique(pairs).size == pairs.size


def test_heavy_rows_terms_and_exceptions():
    heavy = (1, 64, 65, 298)
    hmm = regular_hmm(300, indeg=(3, 4), heavy=heavy, heavy_terms=0.5, heavy_heavy=3, self_loops=True, seed=43)
    deg = in_degrees(hmm)
    light = [j for j in range(300) if j not in heavy]
    assert set(deg[light]) == {3, 4}
    assert tuple(np.nonzero(deg > 4)[0]) == heavy
    for h in heavy:
        src = sources(hmm, h)
        assert src & set(heavy) == set(heavy)  # three fellow heavy rows and the self loop: XM = 4 exceptions
        assert len(src - set(heavy)) == 148     # half of the 296 light states
        # general, not uniform: the light terms' weights differ
        w = [float(p) for r, c, p in zip(hmm.trans_rows, hmm.trans_cols, hmm.trans_probs) if int(c) == h]
        assert len(set(w)) > 100
        # some light rows take this heavy row as a source
        assert sum(1 for j in light if h in sources(hmm, j)) >= 3
    full = regular_hmm(300, indeg=(3, 4), heavy=(150,), seed=41)
    assert in_degrees(full)[150] == 299 and 150 not in sources(full, 150)
    assert hmm_pairs_unique(hmm) and hmm_pairs_unique(full)


def test_unreachable_ties_start_and_inf_emissions():
    hmm = regular_hmm(100, S=5, indeg=(2, 3, 4), heavy=(50,), unreachable=(0, 3, 40, 41), start=(9,), seed=64)
    deg = in_degrees(hmm)
    assert tuple(np.nonzero(deg == 0)[0]) == (0, 3, 40, 41)
    assert list(hmm.start_probabilities_cols) == [9]
    assert {0, 3, 40, 41} & set(int(r) for r in hmm.trans_rows)  # they still are sources
    drawn = regular_hmm(200, indeg=(2,), unreachable=7, seed=5)
    dead = np.nonzero(in_degrees(drawn) == 0)[0]
    assert dead.size == 7 and not set(dead) & set(int(c) for c in drawn.start_probabilities_cols)
    ties = regular_hmm(200, indeg=(3, 4), heavy=(0,), ties=True, seed=6)
    for a in (ties.trans_probs, ties.emissions, ties.start_probabilities):
        assert set(np.unique(a)) <= {1.0, 2.0, 3.0}
    inf = regular_hmm(50, S=4, indeg=(2,), heavy=(10,), inf_emis=((10, 1), (10, 3)), seed=7)
    assert np.isinf(inf.emissions[1, 10]) and np.isinf(inf.emissions[3, 10]) and np.isfinite(inf.emissions[0, 10])
    same = regular_hmm(50, S=4, indeg=(2,), heavy=(10,), inf_emis=((10, 1), (10, 3)), seed=7)
    assert np.array_equal(inf.trans_rows, same.trans_rows) and np.array_equal(inf.emissions, same.emissions)


def test_largest_fused_geometry_lds():
    """6144 states at 12 slots x 512 threads is the last geometry under the 160 KB of LDS."""
    assert fused_lds_bytes(12, 512, (12 * 512 + 1 + 4 + 3) // 4 * 4) == 151952
    assert fused_lds_bytes(16, 512, (16 * 512 + 1 + 4 + 3) // 4 * 4) > 160 * 1024


@pytest.mark.parametrize("name", list(fused_cases.CASES))
def test_case_lands_on_its_kernel_instance(name):
    hmm, max_threads, want = fused_cases.build(name)
    assert expected_plan(hmm, max_threads) == want, name
    if want["fused"] and want["family"] > 0:
        R = want["light_terms"]
        deg = in_degrees(hmm)
        assert int((deg > R).sum()) == want["heavy_rows"]
        # the family before it does not fit: more rows above its R than it holds heavy rows
        prev_r, prev_hm = {2: (0, 0), 4: (2, 2), 8: (4, 4), 16: (8, 4)}[R]
        assert R == 2 or int((deg > prev_r).sum()) > prev_hm


def test_every_family_and_slot_count_has_a_case():
    seen = {(w["family"], w["slots"]) for _, _, w in fused_cases.CASES.values() if w["fused"]}
    for fam in (1, 2, 3, 4):
        slots = {s for f, s in seen if f == fam}
        assert 1 in slots and max(slots) >= 8, (fam, slots)
    assert {s for _, s in seen} == {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}
