#!/usr/bin/env python3
"""Headline benchmark: M state-updates/s (states x observations / s) of the Viterbi hot path on
2405.chmm x emit_50_3500_20.ess (BASELINE.json configs[2]), 1..N MI355X.

One step = one pass of the (min,+) Viterbi step kernel over the whole batch (50 sequences x 3500
observations x 2407 states = 421,225,000 state-updates per GPU), inputs resident in HBM.

Multi-GPU (one process per GPU): `--gpus N` without a torchrun environment re-launches this
script under `torch.distributed.run` (a child process started before anything touches the GPU)
and exits with its code; under torchrun WORLD_SIZE must equal N.
  * default (`--shard none`, weak scaling): every rank runs the whole 50-sequence reference file
    (and, with --replicate R, R-1 rank-seeded synthetic copies of it), no data-path collective;
  * `--shard emit50` / `--shard covid` (strong scaling; covid = BASELINE config 5): the file's
    sequences are LPT-assigned to the ranks (spec_viterbi_amd.sharding), each rank runs its share,
    and the scores are gathered to rank 0 with one RCCL gather after the timed region.
The timed region is bracketed by barrier + synchronize on every rank, the max over ranks is
reported, and value = state-updates of all ranks / that time.

Rank 0 prints ONE JSON line.  A plain run does only what that line's headline needs: set up, warm
up, time `--steps` passes, write the last pass's outputs with `--dump-outputs DIR` (scores.npy,
best_states.npy, with --paths also paths.npy and path_offsets.npy; the inputs are the same in
every run with the same arguments) and print metric / value / ms_per_step, the config and the
HIP-event `timing.kernel_ms` of the timed passes.

`--full` adds everything else.  Every rank checks the reference file's rows of its timed output
bit-exact against committed digests (tests/golden/score_digests.json: SHA-256 of the oracle's
float32 rows), rank 0 also the gathered rows; a mismatch on any rank makes every rank exit
non-zero.  Extra objects: `roofline` (the dominant kernel: HIP-event time on the stream it runs
on; VALU-issue utilisation and HBM bytes from rocprofv3 PMC passes this script runs as child
processes on tools/launch.py with the same workload), the rest of `timing` (setup-inclusive and
host-to-host rates) and `cpu_baseline` (the oracle on this host's cores).
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "data")

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
CLOCK_GHZ = 2.4         # MI355X_MICROARCH.md: max shader clock
KERNEL_NAMES = {1: "fused", 2: "generic", 3: "band", 4: "chain", 5: "pipe", 6: "pipew", 7: "spec2", 8: "spec2-pipe",
                9: "diag"}


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--level", type=int, default=0, help="0 = non-spec (headline); >=2 = _spec path")
    p.add_argument("--model", default="2405.chmm")
    p.add_argument("--ess", default="emit_50_3500_20.ess")
    p.add_argument("--shard", default="none", choices=["none", "covid", "emit50"],
                   help="none: weak scaling (the whole file on every rank); covid / emit50: strong scaling of "
                        "2405 x covid-19.ess / emit_50_3500_20.ess (LPT shares, one RCCL gather)")
    p.add_argument("--kernel", type=int, default=0, help="0 auto, 1 fused, 2 generic")
    p.add_argument("--max-threads", type=int, default=0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 PMC child passes")
    p.add_argument("--no-check", action="store_true", help="skip the golden check (diagnostic ablations only)")
    p.add_argument("--paths", action="store_true", help="also decode paths (backpointers + traceback) every step")
    p.add_argument("--replicate", type=int, default=1,
                   help="batch = the file's sequences plus R-1 same-shape synthetic copies per GPU (full-chip "
                        "weak scaling, SURVEY 8(e): emit_50 x 8k sequences = --replicate 160); 1 = the headline")
    p.add_argument("--full", action="store_true",
                   help="also everything beyond the headline figure: the golden check of the timed output, setup and "
                        "host-to-host timings, the roofline (rocprofv3 PMC child passes, the latency plan's floor) and "
                        "the CPU baseline; --no-cpu-baseline / --no-pmc / --no-check / --cpu-seconds refine it")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last one computed as DIR/<name>.npy: scores (float32), "
                        "best_states (float64), with --paths also paths (float64, the sequences' paths end to end); "
                        "ranks > 0 write <name>_rank<r>.npy; outputs over 64 MB in all: a fixed seeded sample of rows")
    p.add_argument("--dry-run", action="store_true",
                   help="no GPU: exercise the launcher / rendezvous / timing scaffolding over gloo (CPU tests)")
    p.add_argument("--dry-run-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ---- multi-process launch ----------------------------------------------------------------------
def relaunch_under_torchrun(args, argv) -> int:
    """`--gpus N` outside torchrun: start torch.distributed.run as a child (nothing here has
    touched the GPU) with N ranks on 127.0.0.1, return its exit code."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd)


def dist_setup(args):
    """(world, rank, local) from the torchrun environment; process group initialised for N > 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not args.dry_run:
        import torch

        torch.cuda.set_device(local)  # before the RCCL communicator is created
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group("gloo" if args.dry_run else "nccl", init_method="env://")
    return world, rank, local


def barrier(world, args):
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
    if not args.dry_run:
        import torch

        torch.cuda.synchronize()


def max_over_ranks(x: float, world, local, args) -> float:
    if world == 1:
        return x
    import torch
    import torch.distributed as dist

    t = torch.tensor([x], dtype=torch.float64, device="cpu" if args.dry_run else f"cuda:{local}")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ---- accounting --------------------------------------------------------------------------------
def algorithmic_bytes_per_step(n: int, nnz: int) -> int:
    """streamed-CSR bytes of one observation of one sequence:
    8*nnz (value + index) + 4*(n+1) (row pointers) + 4n (emission row) + 4n (read v) + 4n (write v)."""
    return 8 * nnz + 4 * (n + 1) + 12 * n


def algorithmic_bytes_per_launch(n: int, nnz: int, lengths, level: int, paths: bool) -> int:
    """Bytes one launch must move under SURVEY.md 8(d)'s streamed-CSR model, per sequence of length
    L: level <= 1: (L-1) steps (+ 2n uint16 backpointers per step and 4 B per path entry with
    paths); level >= 2: floor((L-1)/level) dense products (4*n*round_up(n,4) + 8n each, read
    whole) plus the (L-1) % level tail steps."""
    step = algorithmic_bytes_per_step(n, nnz)
    total = 0
    for L in lengths:
        if level >= 2:
            chunks, tail = divmod(L - 1, level)
            total += chunks * (4 * n * ((n + 3) // 4 * 4) + 8 * n) + tail * step
        else:
            total += (L - 1) * step
            if paths:
                total += (L - 1) * 2 * n * 2 + 4 * L
    return total


def host_cpu_info() -> dict:
    info = {"nproc": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)), "cgroup_cpus": None,
            "model": None}
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            info["cgroup_cpus"] = round(int(quota) / int(period), 2)
    except (OSError, ValueError):
        pass
    try:
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            if line.startswith("Model name"):
                info["model"] = line.split(":", 1)[1].strip()
    except (OSError, subprocess.SubprocessError):
        pass
    return info


def cpu_baseline(hmm, seqs, seconds: float) -> dict:
    """The oracle (C restatement of GraphBLAS_impl, -O2, OpenMP over sequences) on this host:
    all usable cores (CPU affinity, capped by the cgroup quota and by OMP_NUM_THREADS) over the
    full batch, median of passes for ~`seconds`; then 1 thread over the full batch once."""
    from oracle import oracle

    host = host_cpu_info()
    usable = host["affinity"]
    if host["cgroup_cpus"]:
        usable = min(usable, max(1, int(host["cgroup_cpus"])))
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        usable = min(usable, int(os.environ["OMP_NUM_THREADS"]))
    n = hmm.states_num
    work = n * sum(int(s.size) for s in seqs)
    times, used = [], 1
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or not times:
        t0 = time.perf_counter()
        _, used = oracle.viterbi_batch(hmm, seqs, nthreads=usable)
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    t0 = time.perf_counter()
    oracle.viterbi_batch(hmm, seqs, nthreads=1)
    t1 = time.perf_counter() - t0
    return {
        "value": round(work / med / 1e6, 2), "unit": "M state-updates/s", "cores": int(used), "kind": "port",
        "one_thread": round(work / t1 / 1e6, 2),
        "sample": f"oracle/viterbi_oracle.c (GraphBLAS_impl restatement, -O2) over the full {len(seqs)}-sequence "
                  f"batch: median of {len(times)} passes on {used} OpenMP threads (usable cores); 1 thread: "
                  f"{work / t1 / 1e6:.1f} M/s over the same batch ({t1:.2f} s)",
        "host": host,
    }


# ---- rocprofv3 PMC passes (children on tools/launch.py) ---------------------------------------
PMC_PASSES = {
    "sq": ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY",
           "SQ_ACTIVE_INST_ANY", "SQ_WAIT_INST_ANY", "GRBM_GUI_ACTIVE"],
    "fetch": ["FETCH_SIZE"],
    "write": ["WRITE_SIZE"],
    # where waves wait on LDS (optional: a failed pass drops only these counters)
    "lds": ["SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_LDS", "SQ_ACTIVE_INST_LDS", "SQ_INSTS_LDS_LOAD",
            "SQ_INSTS_LDS_STORE", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_ADDR_CONFLICT"],
}
PMC_OPTIONAL = {"lds"}


def pmc_counters(launch_args: list[str], kernel_prefix: str, kernel_suffix: str = "") -> dict | None:
    """Per-launch counters of the dominant kernel from separate rocprofv3 --pmc passes over
    tools/launch.py (same workload), or None when rocprofv3 is unavailable or a pass fails."""
    import csv
    import glob

    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    out: dict[str, float] = {}
    with tempfile.TemporaryDirectory(prefix="svh_pmc_") as d:
        for name, counters in PMC_PASSES.items():
            # counters through a .txt input file (-i): rocprofv3 then starts the workload as its
            # child process instead of exec'ing it from its own Python launcher (an exec the GPU
            # box refuses and logs in gpurun_out/.graft_exec_refused); one pass per file
            job = os.path.join(d, f"{name}.txt")
            with open(job, "w") as fh:
                fh.write("pmc: " + " ".join(counters) + "\n")
            cmd = ["timeout", "-s", "KILL", "120", prof, "-i", job, "-f", "csv", "-d", os.path.join(d, name),
                   "-o", "run", "--", sys.executable, os.path.join(ROOT, "tools", "launch.py"), *launch_args]
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR="/tmp"))
            if r.returncode != 0:
                sys.stderr.write(f"bench.py: rocprofv3 pass {name} failed ({r.returncode}): {r.stderr[-500:]}\n")
                if name in PMC_OPTIONAL:
                    continue
                return None
            per: dict[str, dict] = {}
            for f in glob.glob(os.path.join(d, name, "**", "*counter_collection.csv"), recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        kn = row.get("Kernel_Name", "")
                        if not kn.startswith(kernel_prefix) or (kernel_suffix and kernel_suffix not in kn):
                            continue
                        per.setdefault(row["Counter_Name"], {}).setdefault(row["Dispatch_Id"], 0.0)
                        per[row["Counter_Name"]][row["Dispatch_Id"]] += float(row["Counter_Value"] or 0)
            for c, disp in per.items():
                out[c] = sum(disp.values()) / len(disp)
    return out or None


XCDS = 8  # MI355X_MICROARCH.md: 8 XCDs, each with its own L2


def essential_bytes_per_launch(n: int, S: int, lengths, paths: bool, xcds: int = XCDS) -> int:
    """HBM bytes a launch cannot avoid: the symbols (uint8) in, the scores (fp32) and best states
    (int64) out, the model's folded (eb, ea) tables (S x n float pairs) read once per XCD (each XCD's
    L2 misses on them once: the workgroups that read a table are spread over all 8), and with paths
    the decoded path (int32 per observation).  SURVEY 8(d)'s streamed-CSR bytes are not this
    kernel's bound (it keeps the model and the scores on chip): reported as bytes only."""
    nseq = len(lengths)
    return sum(lengths) + nseq * n * 4 + nseq * 8 + xcds * S * n * 8 + (4 * sum(lengths) if paths else 0)


def spec2_essential_bytes(n: int, S: int, lengths, table_bytes: int, xcds: int = XCDS) -> int:
    """The same for _spec level 2 on chip (spec2.hip): symbols in, scores and best states out, and
    once per XCD the plan's term tables (svh_batch_plan spec_bytes) and the emission rows (S x n
    fp32), which the chunks then re-read from L2."""
    nseq = len(lengths)
    return sum(lengths) + nseq * n * 4 + nseq * 8 + xcds * (table_bytes + S * n * 4)


def roofline(info, plan, nseq, kernel_ms, algo_bytes, pmc, essential_bytes, steps=0) -> dict:
    """VALU-issue roofline of the step kernels (the per-observation step is VALU + LDS work on
    registers; HBM carries only symbols in and scores out).  Capacity of one SIMD-32: one wave64
    VALU instruction per 2 cycles, and at most one per 4 cycles from a single wave
    (MI355X_MICROARCH.md, cycle constants), so a SIMD holding w waves issues min(w/4, 1/2) per
    cycle.  Peak = the SIMDs the launch occupies x that rate x 2.4 GHz; achieved = SQ_INSTS_VALU
    per launch / HIP-event kernel time.  The pipelined kernel runs nseq x pipe_groups workgroups
    of pipe_waves waves; `issue_frac_all` also counts its SALU and LDS instructions, which take a
    wave's issue slot the same way (its bound at one wave per SIMD).  The wide pipelined kernel runs
    ceil(nseq / W) x pipew_blocks workgroups of W waves (threads / 64), one per CU (its LDS)."""
    waves_per_wg = max(1, int(plan["threads"]) // 64)
    pipe = plan["kernel"] in (5, 8)  # 8: level 2 on the pipelined latency plan (same geometry)
    wide = plan["threads"] == info.get("wide_threads") and plan["slots"] == info.get("wide_slots") and nseq > info["cu_count"]
    wg_per_cu = 4 if wide else 1  # launch-bounds occupancy of the wide plan; one WG per CU otherwise
    pipew = plan["kernel"] == 6
    diag = plan["kernel"] == 9
    wgs = nseq * int(info.get("pipe_groups", 1)) if pipe else nseq
    if pipe:
        wg_per_cu = max(1, -(-wgs // max(info["cu_count"], 1)))
    if diag:  # ceil(nseq / W) groups x diag_ranges workgroups of W waves, spread evenly over the CUs
        wgs = -(-nseq // waves_per_wg) * int(info.get("diag_ranges", 1))
        wg_per_cu = max(1, -(-wgs // max(info["cu_count"], 1)))
    if pipew:
        wgs = -(-nseq // waves_per_wg) * int(info.get("pipew_blocks", 1))
        wg_per_cu = 1
    cus = min(info["cu_count"], -(-wgs // wg_per_cu)) if info["cu_count"] else 256
    waves_per_simd = min(8, waves_per_wg * min(wg_per_cu, -(-wgs // max(cus, 1))) / 4.0)
    rate = min(waves_per_simd / 4.0, 0.5)  # wave-instructions per cycle per SIMD
    peak = cus * 4 * rate * CLOCK_GHZ  # G wave-instructions / s
    res = {"bound": "valu_issue", "unit": "G VALU wave-instr/s", "peak": round(peak, 2),
           "achieved": None, "frac": None, "traffic": None, "kernel_ms": round(kernel_ms, 4),
           "occupancy": {"cus": cus, "of_cus": info["cu_count"], "waves_per_simd": waves_per_simd,
                         "workgroups_per_cu": wg_per_cu}}
    egbs = essential_bytes / (kernel_ms * 1e-3) / 1e9
    res["hbm"] = {"essential_bytes": int(essential_bytes), "essential_GBps": round(egbs, 2),
                  "essential_frac": round(egbs / HBM_PEAK_GBS, 6), "peak_GBps": HBM_PEAK_GBS,
                  "measured_bytes": None, "measured_GBps": None, "measured_frac": None,
                  "measured_over_essential": None, "streamed_csr_model_bytes": int(algo_bytes)}
    peak_chip = info["cu_count"] * 4 * 0.5 * CLOCK_GHZ if info["cu_count"] else 256 * 4 * 0.5 * CLOCK_GHZ
    res["peak_chip"] = round(peak_chip, 2)
    res["frac_chip"] = None
    res["issue_frac_all"] = None
    if pmc and "SQ_INSTS_VALU" in pmc:
        ach = pmc["SQ_INSTS_VALU"] / (kernel_ms * 1e-3) / 1e9
        res["achieved"] = round(ach, 2)
        res["frac"] = round(ach / peak, 4)
        # the same against the whole chip's VALU issue (every SIMD at one wave64 instruction per
        # 2 cycles): a launch that idles SIMDs does not look better than it is
        res["frac_chip"] = round(ach / peak_chip, 4)
        res["valu_per_wave"] = round(pmc["SQ_INSTS_VALU"] / max(pmc.get("SQ_WAVES", 1), 1), 1)
        if "SQ_INSTS_SALU" in pmc and "SQ_INSTS_LDS" in pmc:
            allins = pmc["SQ_INSTS_VALU"] + pmc["SQ_INSTS_SALU"] + pmc["SQ_INSTS_LDS"]
            one_wave = cus * 4 * min(waves_per_simd, 1.0) * 0.25 * CLOCK_GHZ  # 1 instr / 4 cycles / wave
            res["issue_all_G_per_s"] = round(allins / (kernel_ms * 1e-3) / 1e9, 2)
            res["issue_frac_all"] = round(res["issue_all_G_per_s"] / max(one_wave, 1e-9), 4) if waves_per_simd <= 1 else None
        if "SQ_WAVE_CYCLES" in pmc and "SQ_WAVES" in pmc:  # quad-cycles
            res["wave_cycles"] = round(4 * pmc["SQ_WAVE_CYCLES"] / pmc["SQ_WAVES"], 0)
            res["wait_frac"] = round(pmc.get("SQ_WAIT_ANY", 0) / pmc["SQ_WAVE_CYCLES"], 4)
            # the three disjoint shares of a wave's cycles (MI355X_MICROARCH.md, PMC slots): issuing,
            # issue stalls (dependencies / pipe busy), parked on s_waitcnt / s_sleep / barriers
            if "SQ_ACTIVE_INST_ANY" in pmc and "SQ_WAIT_INST_ANY" in pmc:
                res["cycle_split"] = {k: round(pmc.get(c, 0) / pmc["SQ_WAVE_CYCLES"], 4) for k, c in
                                      (("active_inst", "SQ_ACTIVE_INST_ANY"), ("wait_inst", "SQ_WAIT_INST_ANY"),
                                       ("wait_any", "SQ_WAIT_ANY"))}
        if "SQ_WAIT_INST_LDS" in pmc and "SQ_WAVE_CYCLES" in pmc:
            # LDS pass: waves' cycles waiting to issue an LDS instruction, LDS-issue cycles, and the
            # bank / address conflict cycles per LDS-issue cycle (all per launch, summed over waves)
            wc = max(pmc["SQ_WAVE_CYCLES"], 1)
            res["lds"] = {"wait_inst_lds_frac": round(pmc["SQ_WAIT_INST_LDS"] / wc, 4),
                          "active_inst_lds_frac": round(pmc.get("SQ_ACTIVE_INST_LDS", 0) / wc, 4),
                          "loads_per_wave": round(pmc.get("SQ_INSTS_LDS_LOAD", 0) / max(pmc.get("SQ_WAVES", 1), 1), 1),
                          "stores_per_wave": round(pmc.get("SQ_INSTS_LDS_STORE", 0) / max(pmc.get("SQ_WAVES", 1), 1), 1),
                          "bank_conflict_per_active": round(pmc.get("SQ_LDS_BANK_CONFLICT", 0) / max(pmc.get("SQ_ACTIVE_INST_LDS", 1), 1), 4),
                          "addr_conflict_per_active": round(pmc.get("SQ_LDS_ADDR_CONFLICT", 0) / max(pmc.get("SQ_ACTIVE_INST_LDS", 1), 1), 4)}
        if "GRBM_GUI_ACTIVE" in pmc:
            res["profiled_clock_ghz"] = round(pmc["GRBM_GUI_ACTIVE"] / 8 / (kernel_ms * 1e6), 3)
        if diag and "SQ_INSTS_SALU" in pmc and "SQ_INSTS_LDS" in pmc and "SQ_WAVES" in pmc and steps:
            # the diagonal plan has no exchange: its bound is instruction issue on the SIMDs it
            # occupies. Per wave and step: instructions of each kind; per SIMD: the
            # cycles one instruction took on average (every SIMD holding waves_per_simd waves)
            allins = pmc["SQ_INSTS_VALU"] + pmc["SQ_INSTS_SALU"] + pmc["SQ_INSTS_LDS"]
            waves = max(pmc["SQ_WAVES"], 1)
            clk = res.get("profiled_clock_ghz") or CLOCK_GHZ
            simds = cus * 4
            res["issue"] = {"valu_per_step": round(pmc["SQ_INSTS_VALU"] / waves / steps, 2),
                            "salu_per_step": round(pmc["SQ_INSTS_SALU"] / waves / steps, 2),
                            "lds_per_step": round(pmc["SQ_INSTS_LDS"] / waves / steps, 2),
                            "instr_per_step": round(allins / waves / steps, 2),
                            "simd_cycles_per_instr": round(kernel_ms * 1e6 * clk * simds / allins, 2),
                            "note": "per wave and observation step (steps = the longest row's observations - 1); "
                                    "simd_cycles_per_instr = kernel cycles x occupied SIMDs / instructions issued"}
    if pmc and "FETCH_SIZE" in pmc and "WRITE_SIZE" in pmc:  # KiB; FETCH_SIZE doubled on gfx950
        traffic = 2.0 * pmc["FETCH_SIZE"] * 1024 + pmc["WRITE_SIZE"] * 1024
        res["traffic"] = round(traffic)
        mg = traffic / (kernel_ms * 1e-3) / 1e9
        res["hbm"].update(measured_bytes=round(traffic), measured_GBps=round(mg, 2),
                          measured_frac=round(mg / HBM_PEAK_GBS, 6),
                          measured_over_essential=round(traffic / max(essential_bytes, 1), 2))
    res["note"] = ("frac = VALU wave-instructions issued (rocprofv3 SQ_INSTS_VALU, child pass on tools/launch.py) / "
                   "kernel time, over the issue capacity of the SIMDs the launch occupies at its occupancy, at 2.4 GHz; "
                   "frac_chip = the same over the whole chip (CUs x 4 SIMDs x 1/2 per cycle x 2.4 GHz); issue_frac_all = "
                   "VALU + SALU + LDS instructions over one wave's issue rate (1 per 4 cycles) on the occupied SIMDs; "
                   "hbm.essential_* = the bytes a launch cannot avoid (symbols in, scores and best states out, the "
                   "folded tables once per XCD); hbm.measured_* the PMC bytes (FETCH_SIZE x2 + WRITE_SIZE) and their ratio to "
                   "the essential bytes; hbm.streamed_csr_model_bytes = SURVEY 8(d)'s streamed-CSR model (47.98 "
                   "B/state-update), not a bound for a kernel that keeps the model on chip, so no rate is derived from it")
    return res


# ---- workloads ---------------------------------------------------------------------------------
SHARD_FILES = {"covid": "covid-19.ess", "emit50": "emit_50_3500_20.ess"}
DIGESTS = os.path.join(ROOT, "tests", "golden", "score_digests.json")


def digest_rows(model_name: str, ess_name: str):
    """Committed per-row digests of the oracle's scores for this workload, or None."""
    import json as _json

    try:
        with open(DIGESTS) as f:
            return _json.load(f).get(f"{model_name} x {ess_name}")
    except OSError:
        return None


def check_rows(scores, best, index, ref_rows) -> list[int]:
    """Rows q (global indices `index`) whose float32 bytes or best state (unless best is None)
    differ from the digests."""
    import hashlib

    bad = []
    for k, q in enumerate(index):
        row = np.ascontiguousarray(np.asarray(scores[k], np.float32))
        if (hashlib.sha256(row.tobytes()).hexdigest() != ref_rows[q]["scores_sha256"]
                or (best is not None and int(best[k]) != ref_rows[q]["best_state"])):
            bad.append(int(q))
    return bad


DUMP_LIMIT = 64 << 20  # bytes of .npy data per --dump-outputs directory


def dump_outputs(dirname: str, rank: int, scores, best, paths=None) -> None:
    """--dump-outputs: the arrays of the last timed step as DIR/<name>.npy (rank 0) or
    DIR/<name>_rank<r>.npy: scores float32 [rows, n], best_states float64 [rows], with paths the
    rows' decoded paths end to end as float64 (and path_offsets, where row k's path starts).  Over
    DUMP_LIMIT bytes: the same seeded sample of rows in every run, sorted, listed in rows.npy."""
    scores = np.asarray(scores, np.float32)
    nrows = scores.shape[0]
    per_row = scores.shape[1] * 4 + 8 + 8
    if paths is not None:
        per_row += 8 + 8 * max((int(p.size) for p in paths), default=0)
    keep = None
    if nrows * per_row > DUMP_LIMIT:
        keep = np.sort(np.random.default_rng(20240607).choice(nrows, size=max(1, DUMP_LIMIT // per_row), replace=False))
    sel = np.arange(nrows) if keep is None else keep
    arrays = {"scores": np.ascontiguousarray(scores[sel]), "best_states": np.asarray(best)[sel].astype(np.float64)}
    if keep is not None:
        arrays["rows"] = keep.astype(np.float64)
    if paths is not None:
        picked = [np.asarray(paths[k]) for k in sel]
        arrays["paths"] = (np.concatenate(picked) if picked else np.zeros(0)).astype(np.float64)
        arrays["path_offsets"] = np.concatenate([[0], np.cumsum([p.size for p in picked])]).astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + (f"_rank{rank}" if rank else "") + ".npy"), a)


def all_ok(ok: bool, world, local, args) -> bool:
    """Logical AND over ranks (every rank learns whether any rank failed its check)."""
    if world == 1:
        return ok
    import torch
    import torch.distributed as dist

    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cpu" if args.dry_run else f"cuda:{local}")
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return relaunch_under_torchrun(args, argv)
    world, rank, local = dist_setup(args)
    if args.dry_run:
        return dry_run(args, world, rank, local)

    import torch

    import spec_viterbi_amd as svh
    from spec_viterbi_amd.sharding import _gather_rows, gather_scores, lpt_assign

    hmm = svh.read_HMM(os.path.join(DATA, "chmm_files", args.model))
    strong = args.shard != "none"
    ess_name = SHARD_FILES[args.shard] if strong else args.ess
    file_seqs = svh.read_emit_seq(os.path.join(DATA, "ess_files", ess_name))
    assignment = None
    if strong:  # strong scaling: this rank's LPT share of the file
        assignment = lpt_assign([s.size for s in file_seqs], world)
        file_index = list(assignment[rank])
        seqs = [file_seqs[q] for q in file_index]
        data = f"{args.model} + {ess_name} (reference file), LPT-sharded over {world} rank(s)"
    else:  # weak scaling: the whole file on every rank
        file_index = list(range(len(file_seqs)))
        seqs = list(file_seqs)
        data = f"{args.model} + {ess_name} (reference file)" + (f" on each of {world} ranks" if world > 1 else "")
    if args.replicate > 1:
        rng = np.random.default_rng(1000 + rank)
        seqs = list(seqs) + [rng.integers(0, hmm.emit_num, size=s.size).astype(np.uint64)
                             for _ in range(args.replicate - 1) for s in file_seqs]
        data += f"; + {args.replicate - 1} same-shape synthetic copies per rank"
    n = int(hmm.states_num)

    # setup (svh_model_create: host CSR + plans + upload), the counterpart of the per-call model
    # build the reference times inside run_Viterbi (bench_Viterbi.h:53-56, GraphBLAS_impl.cpp:9-54)
    setup = []
    for _ in range(3 if args.full else 0):
        t0 = time.perf_counter()
        m = svh.DeviceModel(hmm, device=local, kernel=args.kernel, max_threads=args.max_threads)
        setup.append(time.perf_counter() - t0)
        m.close()
    model = svh.DeviceModel(hmm, device=local, kernel=args.kernel, max_threads=args.max_threads)
    info = model.info()
    prep_s = None
    if args.level >= 2:  # spec_with, timed apart from the run as bench_Viterbi_spec.h:69-71 does
        torch.cuda.synchronize()
        t_prep = time.perf_counter()
        model.spec_build(args.level)
        torch.cuda.synchronize()
        prep_s = time.perf_counter() - t_prep
    # timing=False: the batch records no events of its own in run() (SVH_BATCH_NO_TIMING): each event
    # record is a marker the next kernel waits behind, ~3 us on MI355X; the timed region below is
    # bracketed by one pair of events on the run's stream instead of a pair per step
    batch = model.batch(seqs, paths=args.paths, timing=False) if seqs else None
    plan = batch.plan(args.level) if batch else info
    # A stream of our own: torch's default stream has handle 0, which the C ABI reads as "the
    # model's own stream", so events recorded on torch's default stream would not bracket the
    # kernel.  Every launch and every event below goes to this one stream.
    stream = torch.cuda.Stream(device=local)
    sptr = stream.cuda_stream
    assert sptr, "expected a non-null HIP stream handle"

    for _ in range(args.warmup):
        if batch:
            batch.run(args.level, sptr)
    torch.cuda.synchronize()

    # HIP events on the stream the kernels run on, bracketing the K timed passes (one record before
    # the first, one after the last: per-step records would put 2 K markers into the timed stream);
    # kernel_ms = that span / K, the average pass on the device, launch gaps included
    ev_start = torch.cuda.Event(enable_timing=True)
    ev_stop = torch.cuda.Event(enable_timing=True)
    barrier(world, args)
    t0 = time.perf_counter()
    ev_start.record(stream)
    for k in range(args.steps):
        if batch:
            batch.run(args.level, sptr)
    ev_stop.record(stream)
    torch.cuda.synchronize()
    barrier(world, args)
    elapsed = max_over_ranks(time.perf_counter() - t0, world, local, args)
    kernel_ms = float(ev_start.elapsed_time(ev_stop)) / max(args.steps, 1)

    scores, best, paths = np.zeros((0, n), np.float32), np.zeros(0, np.int64), None
    if batch and args.paths and args.dump_outputs:
        scores, best, paths = batch.read(sptr, want_paths=True)
    elif batch:
        scores, best = batch.read(sptr)
    if args.dump_outputs and not (strong and world > 1):
        dump_outputs(args.dump_outputs, rank, scores, best, paths)
    # rows of the last timed pass the pipelined kernel handed to the serial kernel (0 expected)
    fallbacks = batch.fallbacks() if batch else 0
    # correctness guard on the timed output: every rank checks the reference file's rows it ran
    # against the committed digests (level <= 1: score_digests.json's non-spec rows; level 2 on the
    # headline file: its level-2 rows, all 50, tests/golden/make_golden.py spec2)
    golden_checked, bad = False, []
    check = args.full and not args.no_check  # the comparison with the reference's rows: --full only
    ref_rows = digest_rows(args.model, ess_name) if check else None
    spec_rows = digest_rows(args.model, f"{ess_name} level {args.level}") if check and args.level >= 2 else None
    if check and args.level <= 1 and ref_rows is not None:
        bad = check_rows(scores[: len(file_index)], best[: len(file_index)], file_index, ref_rows)
        golden_checked = True
    elif check and args.level >= 2 and spec_rows is not None:
        bad = check_rows(scores[: len(file_index)], None, file_index, spec_rows)
        golden_checked = True
    if check and not all_ok(not bad, world, local, args):
        if bad:
            sys.stderr.write(f"bench.py: rank {rank}: timed output differs from the golden digests in rows {bad[:10]}\n")
        return 1
    gathered, gather_ms = None, None
    if strong and world > 1:  # one RCCL gather of the scores (and best states) to rank 0
        t_g = time.perf_counter()
        gathered = gather_scores(assignment, scores, len(file_seqs), n, device=f"cuda:{local}")
        gbest = _gather_rows(assignment, np.asarray(best, np.int64).reshape(-1, 1), len(file_seqs), -1,
                             device=f"cuda:{local}")
        gather_ms = (time.perf_counter() - t_g) * 1e3
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, 0, gathered, gbest.reshape(-1))
        gbad = []
        if rank == 0 and check and args.level <= 1 and ref_rows is not None:
            gbad = check_rows(gathered, gbest.reshape(-1), range(len(file_seqs)), ref_rows)
        if check and not all_ok(not gbad, world, local, args):
            if gbad:
                sys.stderr.write(f"bench.py: gathered rows differ from the golden digests: {gbad[:10]}\n")
            return 1

    if strong:
        total_updates = n * sum(int(s.size) for s in file_seqs)
        updates_per_rank = n * sum(int(s.size) for s in seqs)
    else:
        updates_per_rank = n * sum(int(s.size) for s in seqs)
        total_updates = updates_per_rank * world
    value = total_updates * args.steps / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3

    # host-to-host, rank 0 only, after the timed region: symbols in the device format (packed uint8,
    # what svh_reader_next yields; svh_viterbi_u8: H2D, run, D2H of scores and best states), and
    # from the reader's list of uint64 arrays (svh_viterbi_seqs, narrowed on the host per call)
    e2e_ms = e2e_list_ms = e2e_pageable_ms = None
    if args.full and rank == 0 and seqs and not strong:
        from spec_viterbi_amd.hmm import pack_sequences
        offs, sym64 = pack_sequences(seqs)
        sym8 = sym64.astype(np.uint8)

        def med(f):
            f()
            ts = []
            for _ in range(9):
                t_e = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t_e)
            return float(np.median(ts)) * 1e3
        # results into page-locked arrays (svh_host_alloc): the DMA engine writes them directly
        out = (svh.pinned_empty((len(seqs), n), np.float32), svh.pinned_empty(len(seqs), np.int64))
        e2e_ms = med(lambda: model.viterbi_packed(offs, sym8, level=args.level, paths=args.paths, out=out))
        e2e_pageable_ms = med(lambda: model.viterbi_packed(offs, sym8, level=args.level, paths=args.paths))
        e2e_list_ms = med(lambda: model.viterbi(seqs, level=args.level, paths=args.paths))

    if rank == 0:
        nnz = int(info["nnz"])
        lengths = [int(x.size) for x in seqs]
        algo = algorithmic_bytes_per_launch(n, nnz, lengths, args.level, args.paths)
        spec2 = args.level == 2 and plan["kernel"] == 7  # level 2 on chip (spec2.hip)
        l2pipe = args.level == 2 and plan["kernel"] == 8  # level 2 on the pipelined latency plan
        kname = (KERNEL_NAMES.get(plan["kernel"], "?") + "+traceback" if args.paths
                 else "spec2 (+ step-kernel tail)" if spec2
                 else "spec2-pipe (pipelined level-2 chunks + step-kernel tail)" if l2pipe
                 else "spec_chunk+" + KERNEL_NAMES.get(plan["kernel"], "?") if args.level >= 2
                 else KERNEL_NAMES.get(plan["kernel"], "?"))
        pmc = None
        if args.full and not args.no_pmc and world == 1 and (args.level <= 1 or spec2 or l2pipe) and plan["kernel"] in (4, 5, 6, 7, 8, 9):
            # the dominant kernel's counters (with --paths: the pipelined kernel's PATHS variant, the
            # pass's dominant kernel; its traceback and the exiting chain launch are not counted;
            # level 2: the on-chip chunk kernel, not the step kernels' one-observation tails)
            largs = ["--model", args.model, "--ess", ess_name, "--replicate", str(args.replicate), "--steps", "3",
                     "--warmup", "1", "--level", str(args.level)] + (["--paths"] if args.paths else [])
            kpref = {4: "chain_viterbi_kernel", 5: "pipe_viterbi_kernel", 6: "pipew_viterbi_kernel",
                     7: "spec2_kernel", 8: "pipe_viterbi_kernel", 9: "diag_viterbi_kernel"}[plan["kernel"]]
            # level 2 on the pipelined plan: its L2 instantiation (template argument L2 = true), not the
            # step kernel's one-observation tails that share the name
            pmc = pmc_counters(largs, "void svh::(anonymous namespace)::" + kpref, ", true>" if l2pipe else "")
        # level >= 2 on the dense products streams one product per chunk from HBM: those bytes are
        # its bound; on chip (spec2) the tables are read once per XCD like the step kernels'
        if spec2:
            ess_b = spec2_essential_bytes(n, int(info["S"]), lengths, int(plan["spec_bytes"]))
        elif l2pipe:  # the level-0 plan's tables, read once per XCD, and nothing precomputed
            ess_b = essential_bytes_per_launch(n, int(info["S"]), lengths, False)
        else:
            ess_b = algo if args.level >= 2 else essential_bytes_per_launch(n, int(info["S"]), lengths, args.paths)
        rl = roofline(info, plan, len(seqs), kernel_ms, algo, pmc, ess_b, max(lengths) - 1) if args.full else None
        floor_ms = None
        if args.full and plan["kernel"] == 5 and not args.paths and args.level <= 1 and batch:
            # the latency plan's own floor, measured live: the same launch with every boundary exchange
            # removed (svh_batch_step_floor_ms: each wave sweeps its block with no neighbour input and no
            # waits), i.e. the step's per-observation issue time at one wave per SIMD plus the prologue
            try:
                floor_ms = batch.step_floor_ms(10, sptr)
            except svh._lib.SvhError:  # an A/B geometry without the floor variant (SVH_PIPE_WAVES)
                floor_ms = None
            maxlen = max(lengths)
        if floor_ms is not None:
            rl["latency_frac"] = round(floor_ms / kernel_ms, 4)
            rl["latency"] = {"step_floor_ms": round(floor_ms, 4), "frac": rl["latency_frac"],
                             "floor_ns_per_observation": round(floor_ms * 1e6 / maxlen, 2),
                             "kernel_ns_per_observation": round(kernel_ms * 1e6 / maxlen, 2),
                             "exchange_and_fill_ms": round(kernel_ms - floor_ms, 4),
                             "note": "step_floor = the same pipelined launch with every boundary exchange removed "
                                     "(pipe_kernel.h FLOOR; DESIGN.md 5k); frac = floor / kernel_ms: the share of the "
                                     "pass that is the step itself at one wave per SIMD; the rest is the exchange "
                                     "(instructions, waits) and the fill of the 19-wave chain"}
        workload = (f"{args.model} x {ess_name}" +
                    (f" x{args.replicate} (file sequences + same-shape synthetic copies)" if args.replicate > 1 else "") +
                    (", LPT-sharded (strong scaling)" if strong else "") + ", " +
                    (f"non-spec (min,+) step, {kname} kernel" if args.level <= 1 else f"_spec level {args.level}"))
        out = {
            "metric": f"M state-updates/sec (states x obs/s) on {args.model} x {ess_name}",
            "value": round(value, 2),
            "unit": "M state-updates/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": data,
            "config": {
                "workload": workload, "states": n, "nnz": nnz, "sequences_per_gpu": len(seqs),
                "observations_per_gpu": sum(lengths), "state_updates_per_gpu": updates_per_rank, "level": args.level,
                "kernel": kname, "threads": plan["threads"], "slots": plan["slots"], "paths": bool(args.paths),
                "workgroups_per_sequence": (int(info["pipe_groups"]) if plan["kernel"] == 5 else
                                            int(info["pipew_blocks"]) if plan["kernel"] == 6 else
                                            int(info["diag_ranges"]) if plan["kernel"] == 9 else 1),
                "fallback_rows": fallbacks,
                "heavy_rows": plan["heavy_rows"], "spec_prep_s": None if prep_s is None else round(prep_s, 4),
                "golden_checked": golden_checked,
                "checked_rows": len(file_index) if golden_checked else 0,
                "parallelism": (f"LPT sequence shards x{world}, one RCCL gather of scores after timing" if strong
                                else f"sequence-sharded x{world} (one process per GPU, no collective)"),
            },
            "timing": {"kernel_ms": round(kernel_ms, 4),
                       "gather_ms": round(gather_ms, 3) if gather_ms is not None else None},
        }
        if args.full:  # what took runs of its own: setup and host-to-host timings, roofline, CPU baseline
            out["timing"].update({
                "setup_ms": round(float(np.median(setup)) * 1e3, 3),
                "e2e_ms_per_step": None if e2e_ms is None else round(e2e_ms, 3),
                "e2e_over_kernel_ms": None if e2e_ms is None else round(e2e_ms - kernel_ms, 3),
                "e2e_pageable_out_ms_per_step": None if e2e_pageable_ms is None else round(e2e_pageable_ms, 3),
                "e2e_list_u64_ms_per_step": None if e2e_list_ms is None else round(e2e_list_ms, 3),
                "e2e_M_state_updates_per_s": None if not e2e_ms else round(updates_per_rank / e2e_ms / 1e3, 2),
                "setup_plus_e2e_M_state_updates_per_s": None if not e2e_ms else
                round(updates_per_rank / (e2e_ms + float(np.median(setup)) * 1e3) / 1e3, 2),
                "note": "setup_ms = svh_model_create (host CSR + plans + upload; the reference rebuilds its model inside "
                        "every run_Viterbi call, bench_Viterbi.h:53-56); e2e = svh_viterbi_u8 from host symbols in the device "
                        "format (packed uint8, as svh_reader_next yields them) to host scores and best states in "
                        "page-locked arrays (svh_host_alloc; batch upload, run, D2H straight into them), median of 9 "
                        "on rank 0; e2e_pageable_out = the same into fresh numpy arrays (staged D2H + copy-out); "
                        "e2e_list_u64 = from the reader's list of uint64 arrays (svh_viterbi_seqs, narrowed per "
                        "call), pageable outputs",
            })
            out["roofline"] = rl
        if args.full and not args.no_cpu_baseline and world == 1 and args.level <= 1:
            out["cpu_baseline"] = cpu_baseline(hmm, file_seqs, args.cpu_seconds)
        print(json.dumps(out), flush=True)
    if batch:
        batch.close()
    model.close()
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


def dry_run(args, world, rank, local) -> int:
    """The launcher / rendezvous / barrier / max-over-ranks path with a fixed sleep as the step
    (no GPU): rank r 'runs' for (r+1) ms per step, so the max over ranks is the last rank's.
    With --shard: the file's LPT shares and the post-timing gather of the real path over gloo,
    with stand-in score rows (row q filled with q) that rank 0 checks by position; with
    --dry-run-fail-rank R, rank R reports a failed output check and every rank must exit 1."""
    strong = args.shard != "none"
    for _ in range(args.warmup):
        time.sleep(0.001)
    barrier(world, args)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001 * (rank + 1))
    barrier(world, args)
    elapsed = max_over_ranks(time.perf_counter() - t0, world, local, args)
    if not all_ok(rank != args.dry_run_fail_rank, world, local, args):
        return 1
    out = {"metric": "dry-run", "value": round(world * args.steps / elapsed, 3), "n_gpus": world,
           "steps": args.steps, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
           "scaling": "strong" if strong else "weak"}
    if strong:
        import spec_viterbi_amd as svh
        from spec_viterbi_amd.sharding import _gather_rows, gather_scores, lpt_assign

        file_seqs = svh.read_emit_seq(os.path.join(DATA, "ess_files", SHARD_FILES[args.shard]))
        nseq, width = len(file_seqs), 8
        assignment = lpt_assign([s.size for s in file_seqs], world)
        mine = assignment[rank]
        rows = np.repeat(np.asarray(mine, np.float32).reshape(-1, 1), width, axis=1)
        got = gather_scores(assignment, rows, nseq, width)
        gbest = _gather_rows(assignment, np.asarray(mine, np.int64).reshape(-1, 1), nseq, -1)
        if rank == 0:
            ok = all(np.all(got[q] == q) for q in range(nseq)) and np.array_equal(gbest.reshape(-1), np.arange(nseq))
            out.update(sequences=nseq, shares=[len(a) for a in assignment], gathered_ok=bool(ok))
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
