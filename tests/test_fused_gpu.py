"""GPU: the general path -- the fused step kernels (fused_impl.h: five families x ten slot counts,
scores and decoded paths), the generic kernel and the traceback kernel (misc.hip) -- against the
oracle, bit-exact: scores (-0.0 == +0.0), lowest-index best states, identical paths.

Every case first asserts from svh_model_info / svh_batch_plan that the kernel instance it is meant
to test is the one that runs (tests/fused_cases.py names it; tests/test_helpers_models.py checks the
same expectation on the CPU).  A planner that picks something else fails the case.
"""
import functools

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests import fused_cases
from tests.helpers import (bit_equal, expected_plan, first_mismatch, random_chain_hmm, random_seqs, regular_hmm)

pytestmark = pytest.mark.gpu

PLAN_FIELDS = ("kernel", "family", "slots", "threads", "light_terms", "heavy_rows", "heavy_uniform")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def assert_plan(info, want, what):
    """The plan fields of svh_model_info against an expected_plan-style dict."""
    exp = {k: want[k] for k in PLAN_FIELDS if k != "kernel"}
    exp["kernel"] = _lib.SVH_KERNEL_FUSED if want["fused"] else _lib.SVH_KERNEL_GENERIC
    got = {k: info[k] for k in PLAN_FIELDS}
    print(f"{what}: " + " ".join(f"{k}={got[k]}" for k in PLAN_FIELDS))
    assert got == exp, (what, got, exp)


def names(prefix):
    return [k for k in fused_cases.CASES if k.startswith(prefix)]


def compare(what, scores, best, paths, refs):
    for q, (ref, ref_best, ref_path) in enumerate(refs):
        assert bit_equal(scores[q], ref), (what, q, first_mismatch(scores[q], ref))
        assert best[q] == ref_best, (what, q, best[q], ref_best)
        if paths is not None:
            assert np.array_equal(paths[q], ref_path), (what, q, np.nonzero(paths[q] != ref_path)[0][:5])


def run_model(what, hmm, seqs, want, refs=None, max_threads=0, kernel=_lib.SVH_KERNEL_AUTO, paths=True):
    """Scores pass and decoded-path pass (two kernel instantiations) of one model against the oracle."""
    model = svh.DeviceModel(hmm, kernel=kernel, max_threads=max_threads)
    assert_plan(model.info(), want, what)
    if refs is None:
        refs = [oracle.decode(hmm, s) for s in seqs]
    scores, best = model.viterbi(seqs)
    compare(what + " scores", scores, best, None, refs)
    if paths:
        batch = model.batch(seqs, paths=True)
        # svh_batch_plan distinguishes the two: a model whose scores plan is the uniform family
        # decodes paths on the general plan (argmin ties need the term-by-term form)
        pwant = want
        if want["fused"] and want["heavy_uniform"]:
            pwant = expected_plan(hmm, max_threads, allow_uniform=False)
            assert pwant["fused"] and pwant["family"] == 1, pwant
        assert_plan(batch.plan(), pwant, what + " paths")
        batch.run()
        compare(what + " paths", *batch.read(want_paths=True), refs)
    return model


def run_case(name, lens, **kw):
    hmm, max_threads, want = fused_cases.build(name)
    seqs = random_seqs(int(hmm.emit_num), lens, seed=len(name))
    return run_model(name, hmm, seqs, want, max_threads=max_threads, **kw)


# ---- family x slots ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("fam"))
def test_family_by_slots(name):
    """R2 (general), R4, R8 and R16, each at one slot and at >= 8, every instantiated slot count in
    some family (SM = 16 through max_threads 128 / 256), with two or three general heavy rows."""
    big = fused_cases.CASES[name][2]["slots"] >= 4
    run_case(name, [1, 2, 3, 40, 150] if big else [1, 2, 3, 17, 300])


@pytest.mark.parametrize("L,slots,threads", [(300, 1, 320), (1400, 3, 512)])
def test_r2uni_forced_fused(L, slots, threads):
    """The uniform family, scores only: an MSV-shaped model kept off the chain plans."""
    hmm = random_chain_hmm(L, S=6, seed=L)
    seqs = random_seqs(6, [1, 2, 3, 77, 600], seed=L)
    want = dict(fused=True, family=0, slots=slots, threads=threads, light_terms=2, heavy_rows=2, heavy_uniform=1)
    assert expected_plan(hmm) == want
    model = run_model(f"r2uni_L{L}", hmm, seqs, want, kernel=_lib.SVH_KERNEL_FUSED, paths=False)
    # its decoded paths would take the general R2 plan
    pplan = model.batch(seqs[:1], paths=True).plan()
    assert (pplan["family"], pplan["heavy_uniform"], pplan["slots"]) == (1, 0, slots), pplan


# ---- in-degree boundaries ------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("deg"))
def test_in_degree_boundaries(name):
    """Every light row at exactly R terms (no +inf padding term in any register slot); one row at
    R + 1 becomes a heavy row; five move the model to the next family (past R16: generic)."""
    run_case(name, [1, 2, 3, 17, 200])


# ---- heavy rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("heavy"))
def test_heavy_rows(name):
    """General heavy rows: H = 1, 2, 4 (= HM), full and half degree, exactly XM exception terms
    (fellow heavy rows and self loops), a heavy start state, +inf heavy emissions, exact ties."""
    run_case(name, [1, 2, 3, 4, 17, 300])


# ---- geometry edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("edge"))
def test_geometry_edges(name):
    """n around SM * B, the largest fused model (6143 / 6144 states: 12 slots x 512 threads), the
    first one past it (generic at 1024 threads) and max_threads 64..384 on one 1000-state model."""
    run_case(name, [1, 2, 3, 40])


# ---- symbol-ring refill --------------------------------------------------------------------------
REFILL_LENS = [4092, 4093, 4094, 4095, 4096, 4097, 4100, 8184, 8185, 8186, 8192, 8193]
REFILL_PATH_LENS = [4092, 4093, 4094, 4095, 4096, 4097, 4100]


@functools.lru_cache(maxsize=None)
def refill_refs(name):
    hmm, _, want = fused_cases.build(name)
    seqs = random_seqs(int(hmm.emit_num), REFILL_LENS, seed=7)
    ref, _ = oracle.viterbi_batch(hmm, seqs)
    assert np.isfinite(ref).any(axis=1).all()
    return hmm, want, seqs, [(ref[q], int(np.argmin(ref[q])), None) for q in range(len(seqs))]


@functools.lru_cache(maxsize=None)
def refill_path_refs():
    hmm, _, _ = fused_cases.build("refill_sm1")
    seqs = random_seqs(int(hmm.emit_num), REFILL_PATH_LENS, seed=8)
    return seqs, [oracle.decode(hmm, s) for s in seqs]


@pytest.mark.parametrize("name", ["refill_sm2", "refill_sm1"])
def test_symbol_ring_refill_scores(name):
    """The staged symbols are refilled when i + 3 reaches the ring's end: first at observation 4093,
    then at 8185.  Lengths on both sides of both points."""
    hmm, want, seqs, refs = refill_refs(name)
    run_model(name, hmm, seqs, want, refs=refs, paths=False)


def test_symbol_ring_refill_paths():
    hmm, want, _, _ = refill_refs("refill_sm1")
    seqs, refs = refill_path_refs()
    model = svh.DeviceModel(hmm)
    batch = model.batch(seqs, paths=True)
    assert_plan(batch.plan(), want, "refill_sm1 paths")
    batch.run()
    compare("refill_sm1 paths", *batch.read(want_paths=True), refs)


def test_long_sequences_generic():
    """The generic kernel reads symbols from HBM (no ring); the same lengths, scores and paths."""
    hmm, _, seqs, refs = refill_refs("refill_sm1")
    want = fused_cases.generic(int(hmm.states_num))
    run_model("refill generic", hmm, seqs, want, refs=refs, kernel=_lib.SVH_KERNEL_GENERIC, paths=False)
    pseqs, prefs = refill_path_refs()
    model = svh.DeviceModel(hmm, kernel=_lib.SVH_KERNEL_GENERIC)
    batch = model.batch(pseqs, paths=True)
    assert_plan(batch.plan(), want, "refill generic paths")
    batch.run()
    compare("refill generic paths", *batch.read(want_paths=True), prefs)


# ---- resumed rows --------------------------------------------------------------------------------
# _spec tails begin at 1 + level * chunks: at level 3 the lengths below resume at 1, 4, 7, 10 (every
# residue mod 4), 4096 and 4099 (symbols staged from a late base); at level 2 at 1, 3, 5, 7, 11, 4097
SPEC_LENS = [1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 4098, 4101]


@functools.lru_cache(maxsize=None)
def spec_refs(level):
    hmm, _, want = fused_cases.build("resume_r4")
    seqs = random_seqs(int(hmm.emit_num), SPEC_LENS, seed=9)
    return hmm, want, seqs, oracle.viterbi_spec_batch(hmm, level, seqs)


@pytest.mark.parametrize("forced_generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("level", [2, 3])
def test_spec_tail_resumed_rows(level, forced_generic):
    """The _spec tail: rows resumed at begin > 0 from v_in on the fused (R4) and the generic kernel."""
    hmm, want, seqs, refs = spec_refs(level)
    if forced_generic:
        want = fused_cases.generic(int(hmm.states_num))
    model = svh.DeviceModel(hmm, kernel=_lib.SVH_KERNEL_GENERIC if forced_generic else _lib.SVH_KERNEL_AUTO)
    assert_plan(model.info(), want, f"spec level {level} tail")
    model.spec_build(level)
    got, best = model.viterbi(seqs, level=level)
    for q in range(len(seqs)):
        assert bit_equal(got[q], refs[q]), (q, len(seqs[q]), first_mismatch(got[q], refs[q]))
        assert best[q] == int(np.argmin(refs[q])), q


@functools.lru_cache(maxsize=None)
def timepar_refs():
    hmm, _, want = fused_cases.build("resume_r4")
    seqs = random_seqs(int(hmm.emit_num), [13000, 9000, 100, 1], seed=10)
    ref, _ = oracle.viterbi_batch(hmm, seqs)
    return hmm, want, seqs, ref


@pytest.mark.parametrize("forced_generic", [False, True], ids=["fused", "generic"])
def test_time_parallel_exact_mode_equals_serial(forced_generic):
    """rel_tol < 0 re-runs every segment from its exact start: three segments of 4333 observations
    of the long row, each resumed row refilling its symbol ring; bit for bit the serial pass."""
    hmm, want, seqs, ref = timepar_refs()
    if forced_generic:
        want = fused_cases.generic(int(hmm.states_num))
    model = svh.DeviceModel(hmm, kernel=_lib.SVH_KERNEL_GENERIC if forced_generic else _lib.SVH_KERNEL_AUTO)
    assert_plan(model.info(), want, "time-parallel")
    batch = model.batch(seqs)
    assert batch.run_time_parallel(seg_len=4200, probe_len=256, rel_tol=-1.0) > 0
    scores, best = batch.read()
    one_s, one_b = model.viterbi(seqs)
    assert bit_equal(scores, one_s) and np.array_equal(best, one_b)
    for q in range(len(seqs)):
        assert bit_equal(scores[q], ref[q]), (q, first_mismatch(scores[q], ref[q]))


# ---- generic kernel ------------------------------------------------------------------------------
def test_generic_capacity_edge():
    """20464 states fill the 160 KB of LDS exactly (two score vectors and the reduction scratch);
    the traceback stages one backpointer row per block.  One state more is refused."""
    hmm, _, want = fused_cases.build("generic_capacity")
    assert want["threads"] == 1024
    run_model("generic_capacity", hmm, random_seqs(2, [1, 2, 40], seed=11), want)
    with pytest.raises(_lib.SvhError) as e:
        svh.DeviceModel(regular_hmm(fused_cases.GENERIC_MAX_N + 1, S=2, indeg=(1, 2, 3), seed=66))
    assert e.value.code == _lib.SVH_E_UNSUPPORTED


def test_generic_five_dense_rows():
    """A fifth row of in-degree n: no family holds five heavy rows."""
    run_case("generic_five_dense", [1, 2, 3, 17, 300])


@pytest.mark.parametrize("n", [297, 298, 299])
def test_generic_n_not_a_multiple_of_4(n):
    hmm = regular_hmm(n, indeg=(3, 4), heavy=(5,), zero_emis=0.05, seed=n)
    run_model(f"generic_n{n}", hmm, random_seqs(4, [1, 2, 3, 17, 120], seed=n), fused_cases.generic(n),
              kernel=_lib.SVH_KERNEL_GENERIC)


# ---- traceback -----------------------------------------------------------------------------------
TRACEBACK_LENS = [327, 328, 329, 655, 656, 1, 2]  # 100 states: 327 backpointer rows per staged block


@functools.lru_cache(maxsize=None)
def traceback_refs():
    hmm, _, want = fused_cases.build("traceback_n100")
    S = int(hmm.emit_num)
    live = random_seqs(S - 1, TRACEBACK_LENS, seed=12)  # never the last symbol
    # the last symbol's emission is +inf in every state: every score after it is +inf, the best
    # state is the oracle's lowest index, and the path walks lowest-index predecessors until it
    # meets a state without incoming terms (-1 from there on)
    em = hmm.emissions.copy()
    em[S - 1, :] = np.inf
    hmm.emissions = em
    dead = [s.copy() for s in live[:5]]
    for q, s in enumerate(dead):
        s[[len(s) - 1, len(s) // 2, len(s) - 3, 1, len(s) - 330][q]] = S - 1
    seqs = live + dead
    return hmm, want, seqs, [oracle.decode(hmm, s) for s in seqs]


@pytest.mark.parametrize("forced_generic", [False, True], ids=["fused", "generic"])
def test_traceback_block_edges_and_missing_predecessors(forced_generic):
    hmm, want, seqs, refs = traceback_refs()
    # not vacuous: finite paths, paths with -1 entries after some states, and all-+inf final scores
    assert all((p >= 0).all() for _, _, p in refs[:len(TRACEBACK_LENS)])
    mixed = [p for _, _, p in refs if (p == -1).any()]
    assert len(mixed) >= 3 and any((p[:-1] >= 0).sum() >= 2 for p in mixed)
    assert any(np.isinf(s).all() and b == 0 for s, b, _ in refs)
    if forced_generic:
        want = fused_cases.generic(int(hmm.states_num))
    run_model("traceback", hmm, seqs, want,
              refs=refs, kernel=_lib.SVH_KERNEL_GENERIC if forced_generic else _lib.SVH_KERNEL_AUTO)
