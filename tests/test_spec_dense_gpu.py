"""GPU: the dense `_spec` product path -- spec_fold_kernel, spec_scatter_kernel, spec_extend_kernel
and spec_chunk_kernel (misc.hip), Model::spec_build and the level >= 2 branch of Batch::run
(runtime.cpp) -- against the oracle's GraphBLAS_spec_impl restatement, bit-exact, at levels 2-5.

The reference is oracle.viterbi_spec_batch; tests/test_spec_products.py pins it, on the CPU, to a
second implementation written from the definition.  Every case asserts from svh_model_info that the
dense products were built (spec_bytes is their exact size; the on-chip level-2 kernel reports 0), and
from svh_batch_plan the step kernel of the tail where one is forced.  The batches use every one of
the S^level products at least once (tests/spec_dense_cases.py; asserted before the run), so a product
that is wrong, filed under another key or left unwritten by the extend grid changes some row.

Not covered: spec_chunk_kernel with more than 64 KB of LDS (set_lds_limit, n > 16384 states).  An
oracle product set at that size (S^2 * n^2 * 4 bytes >= 2 GB) does not fit a test of a few seconds.
"""
import functools

import numpy as np
import pytest

import spec_viterbi_amd as svh
from spec_viterbi_amd import _lib
from oracle import oracle
from tests import spec_dense_cases as cases
from tests.helpers import bit_equal, covered_keys, first_mismatch, random_hmm, random_seqs

pytestmark = pytest.mark.gpu

KERNEL = {"auto": _lib.SVH_KERNEL_AUTO, "diag": _lib.SVH_KERNEL_DIAG, "pipe": _lib.SVH_KERNEL_PIPE,
          "pipe_wide": _lib.SVH_KERNEL_PIPE_WIDE, "chain": _lib.SVH_KERNEL_CHAIN, "fused": _lib.SVH_KERNEL_FUSED}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    assert _lib.device_count() > 0, "no HIP device visible (GPU tests must run on an MI355X)"


def names(prefix):
    return [k for k in cases.CASES if k.startswith(prefix)]


def oracle_rows(hmm, level, seqs):
    """The oracle's scores [nseq, n]; at least half of the rows must hold a finite score (a batch
    of +inf rows would pass whatever the products are)."""
    refs = oracle.viterbi_spec_batch(hmm, level, seqs)
    finite = int(np.isfinite(refs).any(axis=1).sum())
    assert 2 * finite >= len(seqs), (finite, len(seqs))
    return refs


def compare(what, got, best, refs):
    """Every row bit-exact (-0.0 == +0.0); best states: the lowest index of the oracle row's minimum
    (ora_argmin's rule; 0 for a row of +inf)."""
    assert got.shape == refs.shape
    if not bit_equal(got, refs):
        q = next(q for q in range(refs.shape[0]) if not bit_equal(got[q], refs[q]))
        raise AssertionError((what, q, first_mismatch(got[q], refs[q])))
    if best is not None:
        want = np.argmin(refs, axis=1)
        bad = np.nonzero(best != want)[0]
        assert bad.size == 0, (what, int(bad[0]), int(best[bad[0]]), int(want[bad[0]]))


def assert_cover(seqs, S, level):
    assert np.array_equal(covered_keys(seqs, S, level), np.arange(S ** level)), (S, level)


def dense_model(hmm, level, kernel=_lib.SVH_KERNEL_AUTO):
    """A model whose level-`level` products are dense in HBM: level 2 by the model flag, deeper
    levels have no other form.  spec_bytes is their exact size."""
    model = svh.DeviceModel(hmm, kernel=kernel, flags=_lib.SVH_MODEL_SPEC_DENSE if level == 2 else 0)
    model.spec_build(level)
    assert_dense(model, level)
    return model


def assert_dense(model, level):
    info = model.info()
    assert info["spec_level"] == level, info
    assert info["spec_bytes"] == cases.spec_bytes(model.n, model.S, level), (info["spec_bytes"], model.n, model.S, level)


@functools.lru_cache(maxsize=1)
def chain_case():
    """The six chain cases share one model and one batch: one oracle run."""
    hmm, level, _, seqs, _ = cases.build("chain_auto")
    assert_cover(seqs, int(hmm.emit_num), level)
    return hmm, level, seqs, oracle_rows(hmm, level, seqs)


def run_case(name):
    if name.startswith("chain_"):
        hmm, level, seqs, refs = chain_case()
        kernel = cases.CASES[name].kernel
    else:
        hmm, level, kernel, seqs, cover = cases.build(name)
        if cover:
            assert_cover(seqs, int(hmm.emit_num), level)
        refs = oracle_rows(hmm, level, seqs)
    model = dense_model(hmm, level, KERNEL[kernel])
    if kernel != "auto":  # the step kernel that runs the tails
        batch = model.batch(seqs)
        plan = batch.plan(level)
        if kernel == "diag":  # at level >= 2 svh_batch_plan names the diagonal tail launch by diag_sm (svh.h)
            assert plan["diag_sm"] in (1, 2), (name, plan)
        else:
            assert plan["kernel"] == KERNEL[kernel], (name, plan["kernel"])
        batch.close()
    got, best = model.viterbi(seqs, level=level)
    compare(name, got, best, refs)
    model.close()


# ---- the cases of tests/spec_dense_cases.py --------------------------------------------------------
@pytest.mark.parametrize("name", names("tile_"))
def test_row_and_column_tiles(name):
    """Level 3 at n = 1 .. 513: one lane, one wave, the chunk kernel's 32 rows per workgroup and its
    clamped rows past n, the padding columns [n, pstride), one to three 256-column tiles of the
    extend kernel; two rows every state leads into."""
    run_case(name)


@pytest.mark.parametrize("name", names("sym_"))
def test_symbol_chunks(name):
    """S around the extend kernel's 32 symbols per workgroup (S = 1 included); at level 3 with
    S = 33 the previous level's 1089 keys and the two symbol chunks share blockIdx.z."""
    run_case(name)


@pytest.mark.parametrize("name", names("deep_"))
def test_levels_4_and_5(name):
    run_case(name)


@pytest.mark.parametrize("name", names("num_"))
def test_numeric_content(name):
    """+inf emissions, product rows that are all +inf with exact ties, negative scores, duplicate
    transitions (the scatter kernel writes one cell per stored term: the first tuple's)."""
    run_case(name)


@pytest.mark.parametrize("name", names("start"))
def test_start_vectors(name):
    """One start state (the chunks read single product columns), two, and every state; level 2 on
    the dense path and level 3."""
    run_case(name)


@pytest.mark.parametrize("name", names("chain_"))
def test_chain_model_tail_under_each_step_kernel(name):
    """An MSV-shaped model of 702 states at level 3: the chunks on the dense products, the tails of
    0, 1 and 2 observations (rows of 256 .. 260 among them) on the forced step kernel."""
    run_case(name)


def test_grid_limit_largest_accepted():
    """S = 127 at level 3: 16129 keys x 4 symbol chunks = 64516 grid planes (the limit is 65535),
    98 MB of products for three states; 300 rows of a key cover."""
    run_case("grid_limit_S127")


def test_grid_limit_refused():
    """S = 128 at level 3 would need 16384 x 4 = 65536 planes."""
    model = svh.DeviceModel(random_hmm(cases.GRID_N, S=128, out_degree=3, dense_rows=(0, 2), seed=128))
    with pytest.raises(_lib.SvhError) as e:
        model.spec_build(3)
    assert e.value.code == _lib.SVH_E_UNSUPPORTED
    info = model.info()
    assert info["spec_level"] == 0 and info["spec_bytes"] == 0, info
    with pytest.raises(_lib.SvhError) as e:
        model.viterbi(random_seqs(128, [5], seed=1), level=3)
    assert e.value.code == _lib.SVH_E_STATE


def test_memory_guard():
    """Level 4 on 4000 states and 20 symbols is 160000 products of 64 MB (about 10 TB): refused with
    SVH_E_NOMEM, nothing built, and the model still runs the plain recurrence bit-exact."""
    hmm = random_hmm(4000, S=20, out_degree=2, seed=40)
    seqs = random_seqs(20, [1, 2, 33, 200], seed=40)
    model = svh.DeviceModel(hmm)
    with pytest.raises(_lib.SvhError) as e:
        model.spec_build(4)
    assert e.value.code == _lib.SVH_E_NOMEM
    info = model.info()
    assert info["spec_level"] == 0 and info["spec_bytes"] == 0, info
    got, best = model.viterbi(seqs)
    refs, _ = oracle.viterbi_batch(hmm, seqs)
    compare("level 0 after the refusal", got, best, refs)


def test_rebuilds_on_one_model_and_one_batch():
    """spec_build replaces any previous products, and a batch object follows the model through the
    levels: its cached chunk counts, tail starts and ping-pong rows are redone when the level (or
    the level-2 form) changes."""
    S, n = 3, 257
    hmm = random_hmm(n, S=S, out_degree=3, dense_rows=(0, n - 1), seed=257)
    seqs = [s for level in (2, 3, 4) for s in cases.default_batch(S, level, seed=50 + level)]
    refs = {}
    for level in (2, 3, 4):
        assert_cover(seqs, S, level)
        refs[level] = oracle_rows(hmm, level, seqs)
    model = svh.DeviceModel(hmm)
    batch = model.batch(seqs)

    def run(level):
        batch.run(level)
        got, best = batch.read()
        compare(f"level {level}", got, best, refs[level])
        return got

    model.spec_build(3)
    assert_dense(model, 3)
    first3 = run(3)
    model.spec_build(2)  # on chip: no products
    assert model.info()["spec_bytes"] == 0 and model.info()["spec_level"] == 2
    chip2 = run(2)
    with pytest.raises(_lib.SvhError) as e:
        batch.run(3)
    assert e.value.code == _lib.SVH_E_STATE
    other = dense_model(hmm, 2)
    dense2, best2 = other.viterbi(seqs, level=2)
    compare("level 2 dense", dense2, best2, refs[2])
    assert bit_equal(dense2, chip2), first_mismatch(dense2, chip2)
    other.close()
    model.spec_build(3)
    assert_dense(model, 3)
    assert bit_equal(run(3), first3)
    model.spec_build(4)
    assert_dense(model, 4)
    run(4)
    run(4)  # the same level again: the cached bookkeeping is reused
    batch.close()
    model.close()


@pytest.mark.parametrize("level", [3, 4])
def test_python_mirror_of_the_reference_interface(level):
    """HIP_spec_impl: spec_with a model, run, spec_with another of a different n and S, run, and the
    first again."""
    hmm_a = random_hmm(65, S=3, out_degree=3, dense_rows=(0, 64), seed=61)
    hmm_b = random_hmm(34, S=2, out_degree=2, dense_rows=(33,), seed=62)
    impl = svh.HIP_spec_impl(level)
    assert impl.get_level() == level
    outs = []
    for hmm in (hmm_a, hmm_b, hmm_a):
        S = int(hmm.emit_num)
        seqs = cases.default_batch(S, level, seed=60 + S)
        assert_cover(seqs, S, level)
        refs = oracle_rows(hmm, level, seqs)
        impl.spec_with(hmm)
        assert_dense(impl._model, level)
        got = impl.run_Viterbi_spec_batch(seqs)
        compare(f"n={hmm.states_num}", got, None, refs)
        one = impl.run_Viterbi_spec(seqs[-1])
        assert bit_equal(one, refs[-1]), first_mismatch(one, refs[-1])
        outs.append(got)
    assert bit_equal(outs[0], outs[2])
