#!/usr/bin/env python3
"""Instruction mix of one kernel of libsmashx from the device assembly (hipcc -S --cuda-device-only):
    python tools/isa_stats.py <mangled-name-substring> [--build] [--account] [--asm FILE] [-D...]
Prints total instruction count and the counts per class (VALU fp32 / fp64 / transcendental / VMEM / SMEM / LDS / SALU / branches / waits).
--account: the vector instructions of the kernel's time loop (the widest backward branch: everything a time block executes, all of its
paths -- general, still and gap regions alike; a STATIC count) split into model arithmetic / compares and selects / copies and
constant moves / exec-mask and lane bookkeeping,.  The loop holds one body of the step per
unrolled step and form (tools say how many: see profiles/vertical_forms_account.md).
--asm FILE reads an assembly file made earlier instead of /tmp/smashx_dev.s."""
import re
import subprocess
import sys
from collections import Counter

ASM = "/tmp/smashx_dev.s"


def build():
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S",
                           "-o", ASM, os.path.join(root, "smash_amd/csrc/smashx.hip")] + [a for a in sys.argv[2:] if a.startswith("-D")],
                          stderr=subprocess.DEVNULL)


def classify(op):
    if op.startswith(("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")): return "valu_trans"
    if op.startswith("v_") and ("f64" in op): return "valu_f64"
    if op.startswith("v_pk_"): return "valu_pk"
    if op.startswith("v_"): return "valu"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")): return "vmem"
    if op.startswith("s_load") or op.startswith("s_buffer"): return "smem"
    if op.startswith("ds_"): return "lds"
    if op.startswith("s_waitcnt"): return "wait"
    if op.startswith(("s_cbranch", "s_branch")): return "branch"
    if op.startswith("s_"): return "salu"
    return "other"


def account_class(op):
    if op.startswith(("v_mov", "v_accvgpr", "v_swap")): return "copies and constant moves"
    if op.startswith(("v_cmp", "v_cndmask")): return "compares and selects"
    if op.startswith(("v_readfirstlane", "v_readlane", "v_writelane", "v_mbcnt")): return "exec-mask and lane bookkeeping"
    if op.startswith("v_"): return "model arithmetic"
    return None


def time_loop(lines):
    """the instructions between the target and the branch of the widest backward branch of the kernel"""
    label = {}
    for i, l in enumerate(lines):
        if l.endswith(":"):
            label[l[:-1]] = i
    best = (0, 0)
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\S+)", l)
        if m and label.get(m.group(1), i) < i and i - label[m.group(1)] > best[1] - best[0]:
            best = (label[m.group(1)], i)
    return [l for l in lines[best[0]:best[1] + 1] if not l.endswith(":")]


def account(dem, text):
    raw = [l.split(";")[0].strip() for l in text.split("\n")]
    raw = [l for l in raw if l and not (l.startswith(".") and not l.endswith(":"))]       # instructions and labels, no directives
    loop = time_loop(raw)
    c = Counter(filter(None, (account_class(l.split()[0]) for l in loop)))
    sx = sum(1 for l in loop if "saveexec" in l.split()[0])
    nconst = sum(1 for l in loop if l.startswith("v_mov_b32") and re.search(r",\s*(0|1\.0|0x7fc00000|-1)$", l))
    total = sum(c.values())
    print(f"{dem[:60]:60s} time loop: {len(loop)} instructions, {total} vector")
    for k in ("model arithmetic", "compares and selects", "copies and constant moves", "exec-mask and lane bookkeeping"):
        print(f"    {k:34s} {c.get(k, 0):5d}  {100.0 * c.get(k, 0) / max(total, 1):5.1f} %")
    print(f"    {'(v_mov of a constant 0 / 1 / NaN / -1)':34s} {nconst:5d}")
    print(f"    {'(scalar: s_*_saveexec regions)':34s} {sx:5d}")


def main():
    if "--build" in sys.argv:
        build()
    asm = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else ASM
    s = open(asm).read()
    key = sys.argv[1]
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", s, re.S | re.M):
        name = m.group(1)
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if key not in name and key not in dem:
            continue
        if "--account" in sys.argv:
            account(dem, m.group(2))
            continue
        lines = [l.strip() for l in m.group(2).split("\n") if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")]
        c = Counter(classify(l.split()[0]) for l in lines)
        print(f"{dem[:70]:70s} total {len(lines):5d}  " + "  ".join(f"{k} {v}" for k, v in sorted(c.items())))


if __name__ == "__main__":
    main()
