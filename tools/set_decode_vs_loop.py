#!/usr/bin/env python3
"""Decoded paths of chosen (model, sequence) pairs: a model set's one decode (svh_batchset_decode)
against the same pairs decoded by hand -- one stand-alone SVH_KERNEL_DIAG path batch per model with
pairs, run back to back --, both on one stream inside one event pair, interleaved rounds in one
process.  One JSON line per cell.

  cell "all"     every reference model x every row of emit_3_3500_20 (72 pairs, 24 members)
  cell "search"  emit_50_3500_20: the set scores every model against every row, then for each row only
                 the pair of its best-scoring model is decoded (50 pairs over a few members)

  (a) loop  every such model's own path batch over its chosen rows (SVH_BATCH_NO_TIMING): four launches each
  (b) set   svh_batchset_decode of the same list

Every pair is checked: against the committed oracle digests where they exist (tests/golden/
scope_digests.json, score_digests.json), otherwise against the CPU oracle's decode; and the set's rows
against the loop's rows bit for bit.

    python3 tools/set_decode_vs_loop.py [--cells all,search] [--rounds 3] [--passes 20]
    python3 tools/set_decode_vs_loop.py --only set --passes 50      (for a profiler: one side alone)
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import spec_viterbi_amd as svh  # noqa: E402
from spec_viterbi_amd import _lib  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.helpers import GOLDEN, bit_equal  # noqa: E402


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype)).tobytes()).hexdigest()


def committed(name, dname):
    """The committed digest rows of (model, dataset), or None."""
    with open(os.path.join(GOLDEN, "scope_digests.json")) as f:
        scope = json.load(f)
    if scope["ess"] == dname and name in scope["models"]:
        return scope["models"][name]
    with open(os.path.join(GOLDEN, "score_digests.json")) as f:
        return json.load(f).get(f"{name} x {dname}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", default="all,search")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--passes", type=int, default=20)
    p.add_argument("--only", default="", choices=["", "set", "loop"])
    a = p.parse_args()
    names = sorted((os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "data", "chmm_files", "*.chmm"))),
                   key=lambda s: int(s.split(".")[0]))
    hmms = [svh.read_HMM(os.path.join(ROOT, "data", "chmm_files", n)) for n in names]
    models = [svh.DeviceModel(h, kernel=_lib.SVH_KERNEL_DIAG) for h in hmms]
    st = torch.cuda.Stream()
    for cell in a.cells.split(","):
        dname = {"all": "emit_3_3500_20.ess", "search": "emit_50_3500_20.ess"}[cell]
        seqs = svh.read_emit_seq(os.path.join(ROOT, "data", "ess_files", dname))
        bs = svh.DeviceModelSet(models).batch(seqs, timing=False)
        if cell == "all":
            pairs = [(m, r) for m in range(len(models)) for r in range(len(seqs))]
        else:  # the search: score the sweep, keep each row's best model
            bs.run(0, st.cuda_stream)
            best = np.stack([s.min(axis=1) for s, _ in bs.read(st.cuda_stream)])  # [models, rows]
            pairs = [(int(best[:, r].argmin()), r) for r in range(len(seqs))]
        chosen = sorted({m for m, _ in pairs})
        rows_of = {m: [r for mm, r in pairs if mm == m] for m in chosen}
        hand = {m: models[m].batch([seqs[r] for r in rows_of[m]], paths=True, timing=False) for m in chosen}

        def loop():
            for b in hand.values():
                b.run(0, st.cuda_stream)

        def one_set():
            bs.decode(pairs, st.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def results(name):
            """[(scores, best, path)] in pair order."""
            if name == "set":
                return bs.read_decoded(st.cuda_stream)
            got = {}
            for m, b in hand.items():
                s, k, pth = b.read(st.cuda_stream, want_paths=True)
                for j, r in enumerate(rows_of[m]):
                    got[(m, r)] = (s[j], int(k[j]), pth[j])
            return [got[pr] for pr in pairs]

        sides = {"loop": loop, "set": one_set}
        if a.only:
            sides = {a.only: sides[a.only]}
        out = {}
        for name, fn in sides.items():
            fn()
            out[name] = results(name)
        checks = []
        for k, (m, r) in enumerate(pairs):
            ref = committed(names[m], dname)
            if ref is None:
                o_scores, o_best, o_path = oracle.decode(hmms[m], seqs[r])
            for name, res in out.items():
                scores, bst, path = res[k]
                if ref is not None:
                    ok = (sha(scores, np.float32) == ref[r]["scores_sha256"] and bst == ref[r]["best_state"] and
                          sha(path, np.int32) == ref[r]["path_sha256"])
                    checks.append("digests" if ok else "MISMATCH")
                else:
                    ok = bit_equal(scores, o_scores) and bst == o_best and np.array_equal(path, o_path)
                    checks.append("oracle" if ok else "MISMATCH")
            if len(out) == 2:
                x, y = out["loop"][k], out["set"][k]
                checks.append("set==loop" if bit_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2]) else "MISMATCH")
        rounds = {name: [] for name in sides}
        for _ in range(a.rounds):
            for name, fn in sides.items():  # interleaved: a round of one side, then of the other
                fn()
                rounds[name].append(statistics.median(timed(fn) for _ in range(a.passes)))
        info = bs.decode_info() if "set" in sides else {}
        rec = {"cell": cell, "dataset": dname, "pairs": len(pairs), "members_with_pairs": len(chosen),
               "loop_launches": 4 * len(chosen), "passes_per_round": a.passes,
               "decode_info": info,
               "ms": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
               "ms_median": {k: round(statistics.median(v), 4) for k, v in rounds.items()},
               "spread": {k: round(max(v) - min(v), 4) for k, v in rounds.items()},
               "fallback_rows_loop": sum(b.fallbacks() for b in hand.values()) if "loop" in sides else None,
               "checks": {c: checks.count(c) for c in sorted(set(checks))}}
        if len(rounds) == 2:
            rec["speedup"] = round(rec["ms_median"]["loop"] / rec["ms_median"]["set"], 2)
        print(json.dumps(rec), flush=True)
        for b in hand.values():
            b.close()
        bs.close()
        if "MISMATCH" in checks:
            raise SystemExit(f"set_decode_vs_loop: {cell}: output check failed")
    for m in models:
        m.close()


if __name__ == "__main__":
    main()
