"""GPU parity of the chain-shaped plans on models whose feeder row N and sink row C sit at any state
index (tests/chain_place_cases.py; tests.helpers.relabel_chain_hmm).

Everywhere else in the suite N = state 0, the light rows are states 1 .. L and C = state L + 1, so
`lrow[p] == p + 1`, `rowF == 0`, `rowS == n - 1`, the feeder wins every best-state tie against a
light row, the sink loses every one, and each tie rule of the decoded paths that compares a heavy
row's index with a light row's has one constant outcome.  Here every chain, band, pipelined, wide
and diagonal kernel scatters (and, in the `_spec` tails, gathers) through row ids that are not the
positions, and the tie rules take their other branches.

Every test is one model and one batch of at most six rows of at most 300 observations (the family C
tests: one model per seed), compared with the oracle bit for bit: scores, the lowest-index best
state, and every path entry.  Every test asserts the plan it meant to run.  A fallback re-runs a row
exactly and would hide a wrong row of the kernel under test: families A, B, D and E assert that no
row fell back (tests/test_chain_place_cases.py establishes on the CPU that none can), family C that
rows did."""
import functools

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests.chain_place_cases import (CASES, PLAN_L, SPEC_L, SPEC_PLACEMENTS, feeder_wins_every_tie, names, placed,
                                     placements, seqs, spec_model, spec_seqs)
from tests.helpers import bit_equal, first_mismatch, relabel_chain_hmm

pytestmark = pytest.mark.gpu
AUTO, CHAIN, BAND = _lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_CHAIN, _lib.SVH_KERNEL_BAND
PIPE, PIPEW, DIAG = _lib.SVH_KERNEL_PIPE, _lib.SVH_KERNEL_PIPE_WIDE, _lib.SVH_KERNEL_DIAG
TODAY = (_lib.SVH_KERNEL_CHAIN, _lib.SVH_KERNEL_FUSED, _lib.SVH_KERNEL_GENERIC)  # a declined path model's route
DIAG_ENV = ("SVH_DIAG_SM", "SVH_DIAG_LOADER", "SVH_DIAG_QUAD")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


# route: (kernel preference, L, SVH_DIAG_* settings read when the model is created, what plan() must say)
ROUTES = {
    "chain": (CHAIN, PLAN_L["chain"], {}, dict(kernel=CHAIN)),
    "band": (BAND, PLAN_L["band"], {}, dict(kernel=BAND)),
    "pipe": (PIPE, PLAN_L["pipe"], {}, dict(kernel=PIPE)),
    "pipew": (PIPEW, PLAN_L["pipew"], {}, dict(kernel=PIPEW)),
    "diag1": (DIAG, PLAN_L["diag"], dict(SVH_DIAG_SM="1"), dict(kernel=DIAG, diag_sm=1)),
    "diag2": (DIAG, PLAN_L["diag"], dict(SVH_DIAG_SM="2", SVH_DIAG_QUAD="0"), dict(kernel=DIAG, diag_sm=2, diag_quad=0)),
    "diag2_130": (DIAG, PLAN_L["diag130"], dict(SVH_DIAG_SM="2", SVH_DIAG_QUAD="0"), dict(kernel=DIAG, diag_sm=2, diag_quad=0)),
    "quad": (DIAG, PLAN_L["diag"], dict(SVH_DIAG_SM="2", SVH_DIAG_LOADER="1", SVH_DIAG_QUAD="1"),
             dict(kernel=DIAG, diag_sm=2, diag_quad=1)),
    "quad_130": (DIAG, PLAN_L["diag130"], dict(SVH_DIAG_SM="2", SVH_DIAG_LOADER="1", SVH_DIAG_QUAD="1"),
                 dict(kernel=DIAG, diag_sm=2, diag_quad=1)),
    "loader1": (DIAG, PLAN_L["diag"], dict(SVH_DIAG_SM="1", SVH_DIAG_LOADER="1"), dict(kernel=DIAG, diag_sm=1)),
    "loader2": (DIAG, PLAN_L["diag"], dict(SVH_DIAG_SM="2", SVH_DIAG_LOADER="1", SVH_DIAG_QUAD="0"),
                dict(kernel=DIAG, diag_sm=2, diag_quad=0)),
    "auto": (AUTO, PLAN_L["chain"], {}, dict(kernel=DIAG)),  # a few rows under AUTO: the diagonal plan
}


def set_env(monkeypatch, env):
    for k in DIAG_ENV:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def assert_plan(plan, want, kernel):
    for k, v in want.items():
        assert plan[k] == v, (k, v, plan)
    if kernel == PIPE:
        assert plan["pipe_groups"] >= 2, plan
    if kernel == PIPEW:
        assert plan["pipew_blocks"] >= 2, plan


@functools.lru_cache(maxsize=None)
def ref_scores(L, name, place):
    """The oracle's rows of one case at one placement, computed once for every route."""
    hmm2, _, _ = placed(CASES[L][name], place)
    return oracle.viterbi_batch(hmm2, seqs(CASES[L][name]))[0]


@functools.lru_cache(maxsize=None)
def ref_decoded(L, name, place):
    hmm2, _, _ = placed(CASES[L][name], place)
    return [oracle.decode(hmm2, s) for s in seqs(CASES[L][name])]


def check_scores(refs, scores, best, tag=()):
    for q in range(len(refs)):
        assert bit_equal(scores[q], refs[q]), tag + (q, first_mismatch(scores[q], refs[q]))
        ref_best = int(np.argmin(refs[q])) if np.isfinite(refs[q]).any() else 0
        assert best[q] == ref_best, tag + (q, best[q], ref_best)


def run_scores(hmm, batch_seqs, kernel):
    model = svh.DeviceModel(hmm, kernel=kernel)
    batch = model.batch(batch_seqs)
    plan = batch.plan()
    batch.run()
    s, best = batch.read()
    fb = batch.fallbacks()
    batch.close()
    model.close()
    return s, best, fb, plan


def run_paths(hmm, batch_seqs, kernel):
    model = svh.DeviceModel(hmm, kernel=kernel)
    batch = model.batch(batch_seqs, paths=True)
    plan = batch.plan()
    batch.run()
    s, best, pth = batch.read(want_paths=True)
    fb = batch.fallbacks()
    batch.close()
    model.close()
    return s, best, pth, fb, plan


def check_decoded(refs, scores, best, pth, tag=()):
    for q, (ref, ref_best, ref_path) in enumerate(refs):
        assert bit_equal(scores[q], ref), tag + (q, first_mismatch(scores[q], ref))
        assert best[q] == ref_best, tag + (q, best[q], ref_best)
        assert np.array_equal(pth[q], ref_path), tag + (q, np.nonzero(pth[q] != ref_path)[0][:5], len(ref_path))


def _params(routes, families, skip=()):
    out = []
    for route in routes:
        L = ROUTES[route][1]
        for name in names(L, families):
            if name in skip:
                continue
            for i, place in enumerate(placements(L)):
                out.append(pytest.param(route, name, i, id=f"{route}-{name}-N{place[0]}C{place[1]}"))
    return out


@pytest.mark.parametrize("route,name,which", _params(ROUTES, "ABDE", skip=("A2", "B2")))
def test_scores(monkeypatch, route, name, which):
    """Scores and best states at level 0: placement x family {A, B, D, E} on every plan; no row of the
    pipelined and diagonal plans fell back."""
    kernel, L, env, want = ROUTES[route]
    place = placements(L)[which]
    set_env(monkeypatch, env)
    hmm2, _, _ = placed(CASES[L][name], place)
    s, best, fb, plan = run_scores(hmm2, seqs(CASES[L][name]), kernel)
    assert_plan(plan, want, kernel)
    assert fb == 0
    check_scores(ref_scores(L, name, place), s, best)


FALLBACK_ROUTES = {"pipe": ROUTES["pipe"], "pipew": ROUTES["pipew"], "diag": (DIAG, PLAN_L["diag"], {}, dict(kernel=DIAG))}


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("route", list(FALLBACK_ROUTES))
def test_scores_fallback_rows(monkeypatch, route, which):
    """Family C: rows fail the check; the in-kernel re-run (latency and diagonal plans) and the chain
    fallback (wide plan) scatter through lrow as well.  Every row matches, and rows did fall back."""
    kernel, L, env, want = FALLBACK_ROUTES[route]
    place = placements(L)[which]
    set_env(monkeypatch, env)
    total = 0
    for name in names(L, "C"):
        hmm2, _, _ = placed(CASES[L][name], place)
        s, best, fb, plan = run_scores(hmm2, seqs(CASES[L][name]), kernel)
        assert_plan(plan, want, kernel)
        check_scores(ref_scores(L, name, place), s, best, (name,))
        total += fb
    assert total > 0


PATH_ROUTES = {"chain": (CHAIN, PLAN_L["chain"]), "pipe": (PIPE, PLAN_L["pipe"]), "pipew": (PIPEW, PLAN_L["pipew"]),
               "diag": (DIAG, PLAN_L["diag"])}


def _path_params(families):
    out = []
    for route, (_, L) in PATH_ROUTES.items():
        for name in names(L, families):
            for i, place in enumerate(placements(L)):
                out.append(pytest.param(route, name, i, id=f"{route}-{name}-N{place[0]}C{place[1]}"))
    return out


@pytest.mark.parametrize("route,name,which", _path_params("ABE"))
def test_paths(monkeypatch, route, name, which):
    """Decoded paths: placement x family {A, B, E} on the chain path variant, the latency plan, the
    wide plan and a SVH_KERNEL_DIAG model.  The diagonal path variant is planned exactly where the
    feeder wins every tie (N below every light row, no dead row); elsewhere plan() names one of
    today's routes."""
    kernel, L = PATH_ROUTES[route]
    case, place = CASES[L][name], placements(L)[which]
    set_env(monkeypatch, {})
    hmm2, _, _ = placed(case, place)
    s, best, pth, fb, plan = run_paths(hmm2, seqs(case), kernel)
    if route != "diag":
        assert_plan(plan, dict(kernel=kernel), kernel)
    elif feeder_wins_every_tie(case, place):
        assert plan["kernel"] == DIAG, plan
    else:
        assert plan["kernel"] in TODAY, plan
    assert fb == 0
    check_decoded(ref_decoded(L, name, place), s, best, pth)


def test_paths_diag_variant_cases():
    """The placements at which family A keeps the diagonal path variant: the control and C first, N
    second; at every other one N sits above a light row."""
    L = PLAN_L["diag"]
    kept = [p for p in placements(L) if feeder_wins_every_tie(CASES[L]["A"], p)]
    assert (0, L + 1) in kept and (1, 0) in kept and (L + 1, 0) not in kept and (64, 65) not in kept


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("route", ["pipe", "pipew"])
def test_paths_fallback_rows(monkeypatch, route, which):
    """Family C with decoded paths on the latency and the wide plan: the rows that fail the check
    run on the chain kernel's path variant and its traceback."""
    kernel, L = PATH_ROUTES[route]
    place = placements(L)[which]
    set_env(monkeypatch, {})
    total = 0
    for name in names(L, "C"):
        hmm2, _, _ = placed(CASES[L][name], place)
        s, best, pth, fb, plan = run_paths(hmm2, seqs(CASES[L][name]), kernel)
        assert_plan(plan, dict(kernel=kernel), kernel)
        check_decoded(ref_decoded(L, name, place), s, best, pth, (name,))
        total += fb
    assert total > 0


# ---- `_spec`: the chunks' kernels scatter by row, the tails read v_in by row
SPEC2_ROUTES = {"spec2": (CHAIN, _lib.SVH_KERNEL_SPEC2), "pipe_l2": (AUTO, _lib.SVH_KERNEL_SPEC2_PIPE),
                "diag_l2": (DIAG, _lib.SVH_KERNEL_SPEC2_DIAG)}


@functools.lru_cache(maxsize=None)
def spec_refs(place, level, lens=None):
    hmm2, _ = relabel_chain_hmm(spec_model(), *place)
    batch_seqs = spec_seqs() if lens is None else [spec_seqs()[-1][:n] for n in lens]
    return hmm2, batch_seqs, [oracle.viterbi_spec(hmm2, level, s) for s in batch_seqs]


@pytest.mark.parametrize("place", SPEC_PLACEMENTS, ids=lambda p: f"N{p[0]}C{p[1]}")
@pytest.mark.parametrize("route", list(SPEC2_ROUTES))
def test_spec_level2(monkeypatch, route, place):
    """`_spec` level 2 of family A (every score non-negative) on spec2_kernel (the chain model), the
    pipelined plan (AUTO) and the diagonal plan (SVH_KERNEL_DIAG): rows of 0, 1, 31 and 150 chunks,
    one-observation tails included."""
    kernel, want = SPEC2_ROUTES[route]
    set_env(monkeypatch, {})
    hmm2, batch_seqs, refs = spec_refs(place, 2)
    model = svh.DeviceModel(hmm2, kernel=kernel)
    model.spec_build(2)
    assert model.info()["spec_bytes"] == 0
    batch = model.batch(batch_seqs)
    assert batch.plan(2)["kernel"] == want, batch.plan(2)
    batch.run(2)
    got, best = batch.read()
    assert batch.fallbacks() == 0
    batch.close()
    model.close()
    check_scores(refs, got, best)


@pytest.mark.parametrize("place", SPEC_PLACEMENTS, ids=lambda p: f"N{p[0]}C{p[1]}")
@pytest.mark.parametrize("kernel", [CHAIN, PIPE, PIPEW, DIAG], ids=["chain", "pipe", "pipew", "diag"])
def test_spec_level3_tail_from_observation_64(monkeypatch, kernel, place):
    """Level 3: 21 chunks on the dense products, then a tail of one and of two observations that the
    step kernel starts at observation 64 from the chunks' scores (v_in, read by row)."""
    set_env(monkeypatch, {})
    hmm2, batch_seqs, refs = spec_refs(place, 3, (65, 66))
    model = svh.DeviceModel(hmm2, kernel=kernel)
    model.spec_build(3)
    assert model.info()["spec_bytes"] > 0
    batch = model.batch(batch_seqs)
    plan = batch.plan(3)
    if kernel == DIAG:  # at level >= 2 svh_batch_plan names the diagonal tail launch by diag_sm (svh.h)
        assert plan["diag_sm"] in (1, 2), plan
    else:
        assert plan["kernel"] == kernel, plan
    batch.run(3)
    got, best = batch.read()
    assert batch.fallbacks() == 0
    batch.close()
    model.close()
    check_scores(refs, got, best)


def test_model_set_of_relabelled_copies(monkeypatch):
    """One set of a control model and two relabelled copies, one batch, one launch: each member
    matches its own oracle, and the copies' scores are the control's at new[...]."""
    set_env(monkeypatch, {})
    L = PLAN_L["diag"]
    case = CASES[L]["B"]
    places = [(0, L + 1), (L + 1, 0), (64, 65)]
    hmms, maps = zip(*[placed(case, p)[:2] for p in places])
    models = [svh.DeviceModel(h) for h in hmms]
    bs = svh.DeviceModelSet(models).batch(seqs(case))
    bs.run()
    res = bs.read()
    info = bs.info()
    assert info["members"] == 3 and info["grouped"] == 3 and info["launches"] == 1, info
    for i, place in enumerate(places):
        assert bs.members[i].plan()["kernel"] == DIAG and bs.members[i].fallbacks() == 0
        check_scores(ref_scores(L, "B", place), res[i][0], res[i][1], (place,))
        for q in range(len(res[i][0])):
            assert bit_equal(res[i][0][q][maps[i]], res[0][0][q]), (place, q)
    bs.close()
    for m in models:
        m.close()


@pytest.mark.parametrize("route", ["pipe", "diag"])
def test_two_batches_rerun(monkeypatch, route):
    """Two batches on one model with N and C interior, each run twice in turn: a second launch
    scatters by row as well."""
    kernel, L = PATH_ROUTES[route]
    place = (64, 65)
    set_env(monkeypatch, {})
    hmm2, _, _ = placed(CASES[L]["A"], place)
    model = svh.DeviceModel(hmm2, kernel=kernel)
    inputs = [seqs(CASES[L]["A"]), seqs(CASES[L]["A2"])]  # (family A: no row of either batch can fall back)
    refs = [oracle.viterbi_batch(hmm2, x)[0] for x in inputs]
    batches = [model.batch(x) for x in inputs]
    for b in batches:
        assert_plan(b.plan(), dict(kernel=kernel), kernel)
    for turn in (0, 1, 0, 1):
        batches[turn].run()
        s, best = batches[turn].read()
        assert batches[turn].fallbacks() == 0
        check_scores(refs[turn], s, best, (turn,))
    for b in batches:
        b.close()
    model.close()
