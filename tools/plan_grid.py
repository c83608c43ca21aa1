#!/usr/bin/env python3
"""The plans the engine reports, over a grid of models, kernel preferences, batch widths, batch
flags and _spec levels: the characterisation that tests/test_plan_grid_gpu.py holds the dispatch
(spec_viterbi_amd/csrc/dispatch.cpp) to.  Nothing runs: the sequences are 3 observations long and
the grid only creates models and batches and asks svh_model_get_info / svh_batch_plan.

One JSON line per cell.  The first line names the fields of svh_model_info; every later line gives
them as a list in that order (the recorded grid stays a small file):

    {"fields": [...]}
    {"model": m, "kernel": k, "status": code}                         model creation refused
    {"model": m, "kernel": k, "spec": l, "info": [...]}               model.info() after spec_build(l) (l = 0: none)
    {"model": m, "kernel": k, "spec": l, "nseq": w, "paths": p, "plan": [...] | "status": code}
                                                                        batch.plan(l) of a batch of w rows

Widths: 1, 2, 4 and both sides of every threshold the model's own info reports (diag_max_nseq,
pipe_max_nseq, pipe_max_nseq_paths, pipew_min_nseq, cu_count).

    python3 tools/plan_grid.py > tests/golden/plan_grid.jsonl      (on the MI355X)
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spec_viterbi_amd as svh  # noqa: E402
from spec_viterbi_amd import _lib  # noqa: E402
from tests.helpers import random_chain_hmm, random_hmm, regular_hmm  # noqa: E402

KERNELS = (_lib.SVH_KERNEL_AUTO, _lib.SVH_KERNEL_FUSED, _lib.SVH_KERNEL_GENERIC, _lib.SVH_KERNEL_BAND,
           _lib.SVH_KERNEL_CHAIN, _lib.SVH_KERNEL_PIPE, _lib.SVH_KERNEL_PIPE_WIDE, _lib.SVH_KERNEL_DIAG)
THRESHOLDS = ("diag_max_nseq", "pipe_max_nseq", "pipe_max_nseq_paths", "pipew_min_nseq", "cu_count")
MAX_WIDTH = 4096  # (a threshold of 0xFFFFFFFF, "always", has no far side worth a batch)
FIELDS = [name for name, _ in _lib.svh_model_info._fields_]


def models():
    """(name, hmm, levels): the last two are small enough for the dense level-3 products."""
    chmm = os.path.join(ROOT, "data", "chmm_files")
    return [
        ("2405.chmm", svh.read_HMM(os.path.join(chmm, "2405.chmm")), (0, 2)),
        ("100.chmm", svh.read_HMM(os.path.join(chmm, "100.chmm")), (0, 2)),
        ("regular_fused", regular_hmm(400, S=4, indeg=(2,), seed=2), (0, 2)),
        ("random_generic", random_hmm(200, S=4, out_degree=30, seed=9), (0, 2)),
        ("chain_one_group", random_chain_hmm(100, S=8, seed=41), (0, 2, 3)),  # <= 512 light rows: one workgroup
        ("chain_S33", random_chain_hmm(30, S=33, seed=33), (0, 2, 3)),  # > 32 symbols: no pipelined plan
    ]


def widths(info: dict) -> list[int]:
    w = {1, 2, 4}
    for name in THRESHOLDS:
        t = int(info[name])
        w.update(x for x in (t - 1, t, t + 1) if 1 <= x <= MAX_WIDTH)
    return sorted(w)


def grid_lines():
    yield json.dumps({"fields": FIELDS})
    for name, hmm, levels in models():
        for kernel in KERNELS:
            key = {"model": name, "kernel": kernel}
            try:
                model = svh.DeviceModel(hmm, kernel=kernel)
            except _lib.SvhError as e:
                yield json.dumps({**key, "status": e.code})
                continue
            ws = widths(model.info())
            batches = {}
            for w in ws:
                seqs = [np.array([(q + t) % hmm.emit_num for t in range(3)], np.uint64) for q in range(w)]
                for paths in (False, True):
                    try:
                        batches[w, paths] = model.batch(seqs, paths=paths)
                    except _lib.SvhError as e:
                        batches[w, paths] = e.code
            for level in levels:
                lkey = {**key, "spec": level}
                if level:
                    try:
                        model.spec_build(level)
                    except _lib.SvhError as e:
                        yield json.dumps({**lkey, "status": e.code})
                        continue
                info = model.info()
                yield json.dumps({**lkey, "info": [info[f] for f in FIELDS]})
                for (w, paths), b in batches.items():
                    cell = {**lkey, "nseq": w, "paths": int(paths)}
                    if isinstance(b, int):
                        yield json.dumps({**cell, "status": b})
                        continue
                    try:
                        plan = b.plan(level)
                        yield json.dumps({**cell, "plan": [plan[f] for f in FIELDS]})
                    except _lib.SvhError as e:
                        yield json.dumps({**cell, "status": e.code})
            for b in batches.values():
                if not isinstance(b, int):
                    b.close()
            model.close()


if __name__ == "__main__":
    for line in grid_lines():
        print(line, flush=True)
