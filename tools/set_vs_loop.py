#!/usr/bin/env python3
"""One dataset against every model: a model set's one run (svh_batchset_run) against the same
member batches run back to back, both on one stream inside one event pair, interleaved rounds in
one process.  One JSON line per dataset.

  (a) loop  every member's own svh_batch_run (SVH_BATCH_NO_TIMING), one after the other
  (b) set   svh_batchset_run on the same members

Every cell is checked: against the committed oracle digests where they exist (bench_sweep.py
digest_rows), otherwise the first sequence against the CPU oracle; and the set's rows against the
loop's rows bit for bit.

    python3 tools/set_vs_loop.py [--datasets emit_3_3500_20.ess,emit_50_3500_20.ess] [--rounds 3] [--passes 20]
    python3 tools/set_vs_loop.py --only set --passes 50      (for a profiler: one side alone)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import spec_viterbi_amd as svh  # noqa: E402
from bench_sweep import digest_rows  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.helpers import bit_equal  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--datasets", default="emit_3_3500_20.ess,emit_50_3500_20.ess")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--passes", type=int, default=20)
    p.add_argument("--only", default="", choices=["", "set", "loop"])
    a = p.parse_args()
    names = sorted((os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "data", "chmm_files", "*.chmm"))),
                   key=lambda s: int(s.split(".")[0]))
    hmms = [svh.read_HMM(os.path.join(ROOT, "data", "chmm_files", n)) for n in names]
    models = [svh.DeviceModel(h) for h in hmms]
    cus = models[0].info()["cu_count"]
    st = torch.cuda.Stream()
    for dname in a.datasets.split(","):
        seqs = svh.read_emit_seq(os.path.join(ROOT, "data", "ess_files", dname))
        bs = svh.DeviceModelSet(models).batch(seqs, timing=False)

        def loop():
            for b in bs.members:
                b.run(0, st.cuda_stream)

        def one_set():
            bs.run(0, st.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def results():
            return [b.read(st.cuda_stream) for b in bs.members]

        sides = {"loop": loop, "set": one_set}
        if a.only:
            sides = {a.only: sides[a.only]}
        out = {}
        for name, fn in sides.items():
            fn()
            out[name] = results()
        checks = []
        for i, n in enumerate(names):
            ref = digest_rows(n, dname, 0)
            for name, res in out.items():
                if ref is not None:
                    ok = all(sha(res[i][0][q]) == ref[q] for q in range(len(seqs)))
                    checks.append("digests" if ok else "MISMATCH")
                else:
                    ok = bit_equal(res[i][0][0], oracle.viterbi(hmms[i], seqs[0]))
                    checks.append("bit-exact" if ok else "MISMATCH")
            if len(out) == 2:
                same = all(bit_equal(out["loop"][i][0][q], out["set"][i][0][q]) for q in range(len(seqs)))
                same = same and np.array_equal(out["loop"][i][1], out["set"][i][1])
                checks.append("set==loop" if same else "MISMATCH")
        fallbacks = sum(b.fallbacks() for b in bs.members)
        rounds = {name: [] for name in sides}
        for _ in range(a.rounds):
            for name, fn in sides.items():  # interleaved: a round of one side, then of the other
                fn()
                rounds[name].append(statistics.median(timed(fn) for _ in range(a.passes)))
        info = bs.info()
        rec = {"dataset": dname, "models": len(names), "sequences": len(seqs), "members": info["members"],
               "grouped": info["grouped"], "launches": info["launches"], "grid": info["grid"], "waves": info["waves"],
               "lds_bytes": info["lds_bytes"], "cus": cus, "workgroups_per_cu": round(info["grid"] / cus, 2),
               "passes_per_round": a.passes,
               "ms": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
               "ms_median": {k: round(statistics.median(v), 4) for k, v in rounds.items()},
               "spread": {k: round(max(v) - min(v), 4) for k, v in rounds.items()},
               "fallback_rows": fallbacks,
               "checks": {c: checks.count(c) for c in sorted(set(checks))}}
        if len(rounds) == 2:
            rec["speedup"] = round(rec["ms_median"]["loop"] / rec["ms_median"]["set"], 2)
        print(json.dumps(rec), flush=True)
        bs.close()
        if "MISMATCH" in checks:
            raise SystemExit(f"set_vs_loop: {dname}: output check failed")
    for m in models:
        m.close()


if __name__ == "__main__":
    main()
