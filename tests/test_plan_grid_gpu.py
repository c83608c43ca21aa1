"""GPU: the plans the engine reports (svh_model_get_info, svh_batch_plan) over tools/plan_grid.py's
grid -- six models, every kernel preference, widths on both sides of every threshold the model
reports, scores and SVH_BATCH_PATHS, levels 0 / 2 / 3 -- against tests/golden/plan_grid.jsonl, the
grid as recorded on the MI355X before the dispatch moved into dispatch.cpp.  Line by line: a change
of any reported field in any cell is a diff here.  The grid creates models and batches of
3-observation sequences and runs nothing."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_grid.jsonl")


@pytest.mark.gpu
def test_plan_grid_matches_the_recorded_grid():
    spec = importlib.util.spec_from_file_location("plan_grid", os.path.join(ROOT, "tools", "plan_grid.py"))
    plan_grid = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plan_grid)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = list(plan_grid.grid_lines())
    diff = [(n + 1, w, g) for n, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} of {len(want)} lines differ; first: line {diff[0][0]}\n  recorded {diff[0][1]}\n  now      {diff[0][2]}"
    assert len(got) == len(want), (len(got), len(want))
