"""CPU: bench.py's multi-process scaffolding (torchrun relaunch, WORLD_SIZE check, barriers,
max-over-ranks timing) with --dry-run over gloo, and its output dump; no GPU is touched, except by
the one test marked gpu (a plain run, in this process)."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def run(*args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=180, env=e)


def test_gpus_2_relaunches_two_ranks():
    r = run("--gpus", "2", "--dry-run", "--steps", "4", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints
    out = lines[0]
    assert out["n_gpus"] == 2 and out["steps"] == 4
    # max over ranks: rank 1 sleeps 2 ms per step
    assert out["ms_per_step"] >= 2.0


def test_gpus_1_runs_in_process():
    r = run("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 1


def test_world_size_mismatch_fails():
    r = run("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


@pytest.mark.parametrize("shard,nseq", [("emit50", 50), ("covid", 16)])
def test_gpus_2_strong_scaling_gathers_every_row(shard, nseq):
    """--shard emit50 / covid at N=2 over gloo: LPT shares of the real file, the post-timing gather
    of score rows and best states, every row placed at its global index on rank 0."""
    r = run("--gpus", "2", "--dry-run", "--shard", shard, "--steps", "2", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")][-1]
    assert out["scaling"] == "strong" and out["sequences"] == nseq and sum(out["shares"]) == nseq
    assert min(out["shares"]) > 0 and out["gathered_ok"] is True


def test_gpus_2_failed_check_on_rank_1_fails_every_rank():
    """A rank whose timed output fails its check makes the whole job exit non-zero (rank 0 prints
    no result line)."""
    r = run("--gpus", "2", "--dry-run", "--dry-run-fail-rank", "1", "--steps", "2", "--warmup", "0")
    assert r.returncode != 0
    assert not [x for x in r.stdout.splitlines() if x.startswith("{")]


def test_digests_agree_with_goldens_and_catch_a_flipped_bit():
    """The committed digests bench.py checks against reproduce the golden rows 0..1 of
    2405 x emit_50 (independently stored as float bit patterns), and one flipped bit in a row is
    caught."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from tests.helpers import from_hex, load_golden

    ref = bench.digest_rows("2405.chmm", "emit_50_3500_20.ess")
    assert len(ref) == 50 and len(bench.digest_rows("2405.chmm", "covid-19.ess")) == 16
    g = load_golden("chmm2405_emit50")["sequences"]
    rows = np.stack([from_hex(r["scores"]) for r in g])
    best = np.array([r["best_state"] for r in g])
    idx = [r["index"] for r in g]
    assert bench.check_rows(rows, best, idx, ref) == []
    rows.view(np.uint32)[1, 7] ^= 1
    assert bench.check_rows(rows, best, idx, ref) == [idx[1]]


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: scores float32, everything else float64, paths end to end with their
    offsets; past the size limit the same sorted sample of rows in every call, named in rows.npy."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(3)
    scores = rng.random((7, 5)).astype(np.float32)
    best = rng.integers(0, 5, size=7)
    paths = [rng.integers(0, 5, size=L).astype(np.int32) for L in (3, 1, 4, 1, 5, 9, 2)]
    d = tmp_path / "all"
    bench.dump_outputs(str(d), 0, scores, best, paths)
    assert sorted(os.listdir(d)) == ["best_states.npy", "path_offsets.npy", "paths.npy", "scores.npy"]
    got = np.load(d / "scores.npy")
    assert got.dtype == np.float32 and got.tobytes() == scores.tobytes()
    assert np.load(d / "best_states.npy").dtype == np.float64 and np.array_equal(np.load(d / "best_states.npy"), best)
    off = np.load(d / "path_offsets.npy").astype(int)
    flat = np.load(d / "paths.npy")
    assert flat.dtype == np.float64 and off[-1] == flat.size
    assert all(np.array_equal(flat[off[k]:off[k + 1]], paths[k]) for k in range(7))

    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * (5 * 4 + 16))  # room for 3 rows of scores + best
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), 0, scores, best)
    bench.dump_outputs(str(b), 1, scores, best)
    rows = np.load(a / "rows.npy").astype(int)
    assert rows.size == 3 and np.all(np.diff(rows) > 0) and np.array_equal(rows, np.load(b / "rows_rank1.npy"))
    assert np.array_equal(np.load(a / "scores.npy"), scores[rows])
    assert np.array_equal(np.load(a / "best_states.npy"), best[rows])
    assert sum(os.path.getsize(a / f) - 128 for f in ("scores.npy", "best_states.npy", "rows.npy")) <= bench.DUMP_LIMIT


def test_steps_must_be_positive():
    r = run("--gpus", "1", "--dry-run", "--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_output(tmp_path, capsys):
    """A plain run prints the headline line without the --full objects, runs exactly --steps timed
    passes, and --dump-outputs holds the timed output: all 50 rows of 2405 x emit_50 equal to the
    committed digests."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - out["config"]["state_updates_per_gpu"] / out["ms_per_step"] / 1e3) <= 1e-3 * out["value"]
    assert "roofline" not in out and "cpu_baseline" not in out and "setup_ms" not in out["timing"]
    assert out["config"]["golden_checked"] is False
    scores, best = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "best_states.npy")
    assert scores.dtype == np.float32 and scores.shape == (50, 2407) and best.dtype == np.float64
    ref = bench.digest_rows("2405.chmm", "emit_50_3500_20.ess")
    assert bench.check_rows(scores, best, range(50), ref) == []
