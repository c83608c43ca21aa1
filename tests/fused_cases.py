"""The models of tests/test_fused_gpu.py and the kernel instance each one is meant to run.

Kept apart from the GPU tests so that tests/test_helpers_models.py can check, without a device, that
every model still lands on the family, slot count and workgroup size its case names (the planner's
rules restated in tests/helpers.py expected_plan); the GPU tests assert the same fields from
svh_model_info.  A case: id -> (model builder, max_threads, expected plan fields).
"""
from tests.helpers import random_hmm, regular_hmm

R_OF = {1: 2, 2: 4, 3: 8, 4: 16}  # general family -> light terms
FAM_OF_R = {2: 1, 4: 2, 8: 3, 16: 4}


def light_set(R):
    """In-degrees that need family R: above the family before it, up to R."""
    return tuple(range(R // 2 + 1, R + 1))


def fused(fam, slots, threads, heavy, uniform=0):
    return dict(fused=True, family=fam, slots=slots, threads=threads, light_terms=2 if fam == 0 else R_OF[fam],
                heavy_rows=heavy, heavy_uniform=uniform)


def generic(n):
    return dict(fused=False, family=-1, slots=0, threads=min(1024, (n + 63) // 64 * 64), light_terms=0, heavy_rows=0,
                heavy_uniform=0)


CASES = {}


def case(name, build, expect, max_threads=0):
    assert name not in CASES
    CASES[name] = (build, max_threads, expect)


# ---- family x slots: (family, n, max_threads, slots, threads) -----------------------------------
FAMILY_SLOTS = [
    (1, 500, 0, 1, 512), (1, 1000, 0, 2, 512), (1, 2500, 0, 5, 512), (1, 4000, 0, 8, 512), (1, 1600, 128, 16, 128),
    (2, 500, 0, 1, 512), (2, 1500, 0, 3, 512), (2, 2000, 0, 4, 512), (2, 6144, 0, 12, 512),
    (3, 500, 0, 1, 512), (3, 1000, 0, 2, 512), (3, 3000, 0, 6, 512), (3, 4000, 0, 8, 512), (3, 4096, 256, 16, 256),
    (4, 500, 0, 1, 512), (4, 2500, 0, 5, 512), (4, 5000, 0, 10, 512), (4, 6144, 0, 12, 512),
]
for fam, n, mt, sm, B in FAMILY_SLOTS:
    R = R_OF[fam]
    if fam == 1:  # two general heavy rows at their exception capacity (XM = 2: the other one and a self loop)
        kw = dict(heavy=(7, n - 2), heavy_terms=1.0 if n <= 1000 else 0.5, heavy_heavy=1, self_loops=True)
    else:
        kw = dict(heavy=(0, n // 2, n - 1), heavy_terms=1.0 if n <= 1000 else 0.5, heavy_heavy=1)
    case(f"fam{fam}_sm{sm}_n{n}",
         lambda n=n, R=R, kw=kw, fam=fam: regular_hmm(n, S=6, indeg=light_set(R), zero_emis=0.03, seed=100 * fam + n % 97,
                                                      **kw),
         fused(fam, sm, B, len(kw["heavy"])), mt)

# ---- in-degree boundaries: every light row at exactly R; one row at R + 1 (heavy); five rows at
#      R + 1 (the next family; past R16 the generic kernel) ---------------------------------------
BOUNDARY_N = 333


def _boundary(R, extra, seed):
    """Every row has exactly R terms; `extra` rows get one more."""
    import numpy as np

    from spec_viterbi_amd import HMM

    hmm = regular_hmm(BOUNDARY_N, S=5, indeg=(R,), zero_emis=0.03, seed=seed)
    rng = np.random.default_rng(seed + 1)
    rows, cols, probs = list(hmm.trans_rows), list(hmm.trans_cols), list(hmm.trans_probs)
    for j in rng.choice(BOUNDARY_N, size=extra, replace=False):
        have = set(int(r) for r, c in zip(hmm.trans_rows, hmm.trans_cols) if int(c) == int(j))
        k = next(int(x) for x in rng.permutation(BOUNDARY_N) if int(x) not in have)
        rows.append(k), cols.append(int(j)), probs.append(np.float32(rng.uniform(0.1, 4.0)))
    return HMM(states_num=BOUNDARY_N, emit_num=5, trans_num=len(probs), trans_rows=np.array(rows, np.uint64),
               trans_cols=np.array(cols, np.uint64), trans_probs=np.array(probs, np.float32), emissions=hmm.emissions,
               start_probabilities_cols=hmm.start_probabilities_cols, start_probabilities=hmm.start_probabilities)


for R in (2, 4, 8, 16):
    fam = FAM_OF_R[R]
    B = 384  # 333 states, one slot
    case(f"deg{R}_exact", lambda R=R: _boundary(R, 0, 10 + R), fused(fam, 1, B, 0))
    # R2: a heavy row of three distinct weights is "uniform" (one dominant term, two exceptions), so
    # the scores plan is R2Uni and the path plan the general R2 family
    case(f"deg{R}_one_above", lambda R=R: _boundary(R, 1, 20 + R),
         fused(0, 1, B, 1, uniform=1) if R == 2 else fused(fam, 1, B, 1))
    case(f"deg{R}_five_above", lambda R=R: _boundary(R, 5, 30 + R),
         generic(BOUNDARY_N) if R == 16 else fused(fam + 1, 1, B, 0))

# ---- heavy rows --------------------------------------------------------------------------------
case("heavy_r4_h1", lambda: regular_hmm(300, indeg=(3, 4), heavy=(150,), self_loops=True, seed=41), fused(2, 1, 320, 1))
case("heavy_r4_h2_half", lambda: regular_hmm(300, indeg=(3, 4), heavy=(0, 299), heavy_terms=0.5, heavy_heavy=1, seed=42),
     fused(2, 1, 320, 2))
# four heavy rows, each with exactly XM = 4 exception terms (three fellow heavy rows and a self loop)
case("heavy_r4_h4_xm", lambda: regular_hmm(300, indeg=(3, 4), heavy=(1, 64, 65, 298), heavy_heavy=3, self_loops=True,
                                            seed=43), fused(2, 1, 320, 4))
case("heavy_r8_h4_xm", lambda: regular_hmm(700, indeg=(5, 8), heavy=(0, 383, 384, 699), heavy_terms=0.5, heavy_heavy=3,
                                            self_loops=True, seed=44), fused(3, 2, 384, 4))
case("heavy_r2_h2_xm", lambda: regular_hmm(300, indeg=(1, 2), heavy=(5, 200), heavy_heavy=1, self_loops=True, seed=45),
     fused(1, 1, 320, 2))
# a heavy row that is a start state, and one whose emission is +inf for two of the four symbols
case("heavy_start_inf", lambda: regular_hmm(300, indeg=(3, 4), heavy=(10, 130), heavy_heavy=1, self_loops=True,
                                             start=(10, 77), inf_emis=((130, 0), (130, 2), (10, 1)), seed=46),
     fused(2, 1, 320, 2))
# exact ties everywhere: the lowest-index rule through lex_key, within a wave and across the 5 / 12 waves
case("heavy_ties_r4", lambda: regular_hmm(300, indeg=(3, 4), heavy=(2, 170), heavy_heavy=1, self_loops=True, ties=True,
                                           seed=47), fused(2, 1, 320, 2))
case("heavy_ties_r8_sm2", lambda: regular_hmm(700, indeg=(5, 8), heavy=(300, 301, 650), heavy_heavy=2, ties=True,
                                               zero_emis=0.05, seed=48), fused(3, 2, 384, 3))
case("heavy_ties_r16_sm10", lambda: regular_hmm(5000, indeg=light_set(16), heavy=(0, 511, 512, 4999), heavy_terms=0.5,
                                                 heavy_heavy=3, self_loops=True, ties=True, seed=50), fused(4, 10, 512, 4))
case("heavy_ties_r2", lambda: regular_hmm(300, indeg=(1, 2), heavy=(0, 299), heavy_heavy=1, ties=True, seed=49),
     fused(1, 1, 320, 2))

# ---- geometry edges ----------------------------------------------------------------------------
for n, sm, B in [(63, 1, 64), (64, 1, 64), (65, 1, 128), (511, 1, 512), (512, 1, 512), (513, 2, 320), (1024, 2, 512),
                 (1025, 3, 384), (6143, 12, 512)]:
    case(f"edge_n{n}", lambda n=n: regular_hmm(n, indeg=(3, 4), heavy=(n - 1,), heavy_terms=0.5, seed=n),
         fused(2, sm, B, 1))
# (6144 at 12 slots is fam2_sm12_n6144 and fam4_sm12_n6144 above)
case("edge_n6145", lambda: regular_hmm(6145, indeg=(3, 4), heavy=(6144,), heavy_terms=0.5, seed=6145), generic(6145))
for mt, sm in [(64, 16), (128, 8), (256, 4), (384, 3)]:
    case(f"edge_threads{mt}", lambda: regular_hmm(1000, indeg=(3, 4), heavy=(999,), heavy_terms=0.5, seed=1000),
         fused(2, sm, mt, 1), mt)

# ---- models of the longer-running tests ----------------------------------------------------------
case("refill_sm2", lambda: regular_hmm(700, S=8, indeg=(3, 4), heavy=(0, 699), heavy_terms=0.5, heavy_heavy=1,
                                        self_loops=True, seed=61), fused(2, 2, 384, 2))
case("refill_sm1", lambda: regular_hmm(130, S=8, indeg=(3, 4), heavy=(129,), self_loops=True, seed=62),
     fused(2, 1, 192, 1))
case("resume_r4", lambda: regular_hmm(300, S=4, indeg=(3, 4), heavy=(7, 250), heavy_heavy=1, self_loops=True, seed=63),
     fused(2, 1, 320, 2))
# twelve states without incoming terms and one start state; the seed is chosen so that the oracle's
# lowest-index walk from an all-+inf final vector meets such a state after two steps
case("traceback_n100", lambda: regular_hmm(100, S=5, indeg=(2, 3, 4), heavy=(50,), unreachable=12, start=(9,),
                                            seed=64), fused(2, 1, 128, 1))
# the generic kernel's models under AUTO: a fifth dense row (no family holds five heavy rows), and the
# largest model that fits the on-chip score vector
case("generic_five_dense", lambda: random_hmm(300, S=6, out_degree=2, dense_rows=(0, 1, 150, 298, 299), seed=65),
     generic(300))
GENERIC_MAX_N = 20464
case("generic_capacity", lambda: regular_hmm(GENERIC_MAX_N, S=2, indeg=(1, 2, 3), seed=66), generic(GENERIC_MAX_N))


def build(name):
    """(model, max_threads, expected plan) of a case."""
    b, mt, exp = CASES[name]
    return b(), mt, exp
