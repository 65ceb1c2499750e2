#!/usr/bin/env python3
"""Compiled SCHEDULE of the kernels of a gfx950 .s file (hipcc -S --cuda-device-only with the Makefile's flags): per kernel symbol the register
counts and, for every basic block that holds MFMAs, the ORDER of the instructions that matter to the matrix pipe as a run-length string:

    M mfma   d LDS read   w LDS write   g global / buffer load   s global / buffer store   W s_waitcnt   B s_barrier
    E instruction that writes EXEC (s_and_saveexec, s_or_b64 exec, ...)   b branch   (everything else is skipped)

so "M d M d M d" is one gather behind each MFMA and "24d W 18M" a block of gathers in front of a block of MFMAs.  A basic block ends at a label
or a branch: a stage of the weight gradient that is cut by an "E b |" cannot be interleaved by sched_group_barrier, whatever the source says.
usage: asm_schedule.py <file.s> [kernel-name substring] [--min-mfma N]"""
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
min_mfma = int(sys.argv[sys.argv.index("--min-mfma") + 1]) if "--min-mfma" in sys.argv else 1
if "--min-mfma" in sys.argv:
    args.remove(sys.argv[sys.argv.index("--min-mfma") + 1])
path, pat = args[0], (args[1] if len(args) > 1 else "")
lines = open(path).read().split("\n")


def cls(op, rest):
    if op.startswith("v_mfma"): return "M"
    if op.startswith(("ds_read", "ds_load")): return "d"
    if op.startswith(("ds_write", "ds_store")): return "w"
    if op.startswith(("buffer_store", "global_store", "flat_store")): return "s"
    if op.startswith(("buffer_load", "global_load", "flat_load")): return "g"
    if op.startswith("s_waitcnt"): return "W"
    if op.startswith("s_barrier"): return "B"
    if op.startswith(("s_cbranch", "s_branch")): return "b"
    if "saveexec" in op or (op.startswith("s_") and re.match(r"\s*exec\b", rest)): return "E"
    return None


def rle(seq):
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        out.append(("%d%s" % (j - i, seq[i])) if j - i > 1 else seq[i])
        i = j
    return " ".join(out)


starts = [i for i, l in enumerate(lines) if re.match(r"^[_A-Za-z0-9$.]+:", l) and not l.startswith(".") and pat in l
          and i + 1 < len(lines) and any("s_endpgm" in m for m in lines[i:i + 200000])]
kernels = [i for i in starts if any(re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(lines[i].split(":")[0]) + r"\s*$", m) for m in lines)]
for s in kernels:
    name = lines[s].split(":")[0]
    e = next(i for i in range(s, len(lines)) if "s_endpgm" in lines[i])
    regs = {}
    for l in lines[e:e + 400]:
        m = re.match(r"\s*;\s*(NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\S+)", l)
        if m and m.group(1) not in regs:
            regs[m.group(1)] = m.group(2)
    blocks, cur, label = [], [], "entry"
    for l in lines[s + 1:e]:
        t = l.split(";")[0].strip()
        if not t or t.startswith("//"):
            continue
        if re.match(r"^[.A-Za-z0-9_$]+:$", t):
            blocks.append((label, cur)); cur = []; label = t[:-1]
            continue
        if t.startswith("."):
            continue
        parts = t.split(None, 1)
        c = cls(parts[0], parts[1] if len(parts) > 1 else "")
        if c:
            cur.append(c)
        if c == "b":
            blocks.append((label, cur)); cur = []; label = label + "+"
    blocks.append((label, cur))
    total = "".join("".join(b) for _, b in blocks)
    print("== %s" % name)
    print("   registers: %s" % "  ".join("%s %s" % kv for kv in regs.items()))
    print("   whole kernel: %d mfma, %d LDS reads, %d loads, %d waits, %d EXEC writes, %d branches, %d blocks with MFMAs" % (
        total.count("M"), total.count("d"), total.count("g"), total.count("W"), total.count("E"), total.count("b"),
        sum(1 for _, b in blocks if b.count("M") >= 1)))
    for label, b in blocks:
        if b.count("M") >= min_mfma:
            print("   [%s] %d mfma: %s" % (label, b.count("M"), rle(b)))
