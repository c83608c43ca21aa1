#!/usr/bin/env python3
"""Check where the quad-ring kernel's unrolled block issues its LDS reads and waits.

    make build/diag.dev.s
    python3 tools/diag_rdplace_check.py build/diag.dev.s [--kernel SUBSTRING] [--group-reads N]

The block of 64 steps is the stretch of the kernel between two labels or s_barrier instructions that
holds 64 x 4 v_pk_add_f32 (four packed adds per two-diagonal step).  The read placement the build
keeps (diag_body.h block(), SVH_DIAG_RDPLACE = 1) shows in it as follows; the parent order
(SVH_DIAG_RDPLACE = 0) fails the second point, most of its bodies having two or three runs.
  * The s_waitcnt instructions that name lgkmcnt number exactly 32, one per two-step body, and none has
    the count 0 (the first carries a vmcnt as well).
  * The ds_read_* instructions ahead of each of them, a body's reads, are four (two constants, two quads)
    or, every other body, four and the group reads (one; two with X_SF: --group-reads), and they stand in
    ONE run of consecutive instructions -- nothing between two reads.  Two bodies of the 32 may have the
    group reads in a run of their own, right behind the other four: the block's first and the one whose
    group read is the first to go to the next block's stream buffer, where the buffer's base address is
    made (scalar instructions and a move) between the two runs.
  * No read stands behind the last wait.
Prints the figures and exits 1 if one of them is off.  It reads only ds_read, s_waitcnt, s_barrier,
v_pk_add_f32 and labels.

step2_figures() counts what the two-diagonal step whose {F, c} pair advances in place (diag_body.h step2,
SVH_DIAG_S2PAIR = 1) shows in the same block: 64 x 4 v_pk_add_f32, no v_add_f32 and no v_mov_b32 in a
step (--step2 prints them; the build that leaves the pair to the compiler, = 0, has a move per step).
"""
import argparse
import re
import sys

HEADLINE = "diag_viterbi_kernelILi4ELb0ELb0ELi2ELb1ELb0ELb1EE"  # W = 4, two diagonals, loader wave, quad ring


def kernel_text(path, needle):
    lines = open(path).read().split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^(\S+):", line)
        if m and needle in m.group(1) and not m.group(1).startswith("."):
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            return lines[i + 1 : j]
    raise SystemExit(f"no kernel with {needle!r} in {path}")


def block_of(lines, packed=256):
    """The unrolled block: packed = its v_pk_add_f32 count, None = whatever the fullest stretch has."""
    segs = [[]]
    for line in lines:
        t = line.strip()
        if re.match(r"^\.L\w+:", t) or t.startswith("s_barrier"):
            segs.append([])
        elif t and not t.startswith((";", ".")):
            segs[-1].append(t)
    seg = max(segs, key=lambda s: sum(x.startswith("v_pk_add_f32") for x in s))
    n = sum(x.startswith("v_pk_add_f32") for x in seg)
    if packed is not None and n != packed:
        raise SystemExit(f"the fullest stretch has {n} v_pk_add_f32, not {packed}: the block is not unrolled in one piece")
    return seg


def bodies_of(seg):
    """[(runs of consecutive ds_read ahead of the wait, the wait's lgkmcnt)], and the runs behind the last wait."""
    bodies, runs, run = [], [], 0
    for t in seg:
        if t.startswith("ds_read"):
            run += 1
            continue
        if run:
            runs.append(run)
            run = 0
        if t.startswith("s_waitcnt"):
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m:
                bodies.append((runs, int(m.group(1))))
                runs = []
    if run:
        runs.append(run)
    return bodies, runs


def check(path, kernel=HEADLINE, group_reads=1):
    bodies, trailing = bodies_of(block_of(kernel_text(path, kernel)))
    sizes = (4, 4 + group_reads)
    one_run = sum(len(r) == 1 and r[0] in sizes for r, _ in bodies)
    split = sum(r == [4, group_reads] for r, _ in bodies)
    r = {
        "waits": len(bodies),
        "zero_counts": sum(c == 0 for _, c in bodies),
        "counts": sorted(set(c for _, c in bodies)),
        "longest_run": max([x for r, _ in bodies for x in r] + trailing + [0]),
        "bodies_one_run": one_run,
        "bodies_group_apart": split,
        "bodies_other": len(bodies) - one_run - split,
        "reads_behind_last_wait": sum(trailing),
    }
    r["ok"] = (r["waits"] == 32 and r["zero_counts"] == 0 and r["bodies_other"] == 0 and r["bodies_group_apart"] <= 2
               and r["bodies_one_run"] >= 30 and r["reads_behind_last_wait"] == 0)
    return r


def step2_figures(path, kernel=HEADLINE):
    """The block's adds and moves; moves_in_steps: v_mov_b32 between a body's wait and its last v_cmpx."""
    seg = block_of(kernel_text(path, kernel), packed=None)
    in_steps, pending, waited = 0, 0, False
    for t in seg:
        if t.startswith("s_waitcnt") and "lgkmcnt" in t:
            waited, pending = True, 0
        elif waited and t.startswith("v_mov_b32"):
            pending += 1
        elif waited and t.startswith("v_cmpx"):
            in_steps += pending
            pending = 0
    return {
        "packed_adds": sum(t.startswith("v_pk_add_f32") for t in seg),
        "plain_adds": sum(t.startswith("v_add_f32") for t in seg),
        "moves": sum(t.startswith("v_mov_b32") for t in seg),
        "moves_in_steps": in_steps,
        "checks": sum(t.startswith("v_cmpx") for t in seg),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("asm")
    p.add_argument("--kernel", default=HEADLINE)
    p.add_argument("--group-reads", type=int, default=1)
    p.add_argument("--step2", action="store_true", help="print step2_figures() as well")
    a = p.parse_args()
    if a.step2:
        print(step2_figures(a.asm, a.kernel))
    r = check(a.asm, a.kernel, a.group_reads)
    print(r)
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
