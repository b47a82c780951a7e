#!/usr/bin/env python3
"""Times smashx_adjust_interception (adjust_interception_store on the resident forcing) on the headline grids: gr-b, n^2 cells x 8760
steps, compact forcing built on the device block by block as bench.py builds it, default build.  Per size: wall time of the call and
the device time between its first and last launch (the library prints it under SMASHX_VERBOSE; the call's stderr is captured), median
of --reps, 49-candidate cell-steps/s, the bytes of forcing resident per cell-step and the HBM read rate that implies beside what
tools/hbm_probe.py sustains (profiles/r2_hbm_probe.json), the kernel's registers and waves per SIMD (a listing written by
tools/kernel_resources.py), and beside it the reference's rate on one CPU core as tests/golden/make_interception.py --time printed it.

    python tools/interception_bench.py --sizes 1024 2048 --out profiles/interception_1024_2048.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from resident_forcing import CapturedStderr, plan_with_device_forcing, timed      # noqa: E402


def one_size(n, nt, reps, torch, dev):
    m, _, sol, info, setup_s = plan_with_device_forcing(n, nt, 0, torch, dev)
    day = (1 + np.arange(nt) // 24).astype(np.int32)          # pet_hour0 = 0: step 0 is hour 0 of day 1
    ci = np.zeros((n, n), np.float32, order="F")
    t, _ = timed(lambda: sol.adjust_interception(day, ci), r"adjust_interception .*?: (?P<ms>[0-9.]+) ms on the device, (?P<launches>\d+) launches", reps)
    del t["first_call_wall_s"]
    cells = sol.ncells
    sol.close()
    act = np.asarray(m.active_cell) == 1
    wall_s, dev_s = t["wall_s_median"], t["device_s_median"]
    return {"grid": f"{n}x{n}", "cells": cells, "nt": nt, "forcing": info, "setup_s": round(setup_s, 2), "reps": reps, **t,
            "device_s_per_launch": round(dev_s / t["launches"], 4),
            "cellsteps_per_s_wall": cells * nt / wall_s, "cellsteps_per_s_device": cells * nt / dev_s,
            "interception_steps_per_s_device": 49.0 * cells * nt / dev_s,
            "resident_bytes_per_cellstep": info["resident_bytes_per_cellstep"],
            "hbm_read_GBps_if_each_word_is_read_once": round(info["resident_bytes_per_cellstep"] * cells * nt / dev_s * 1e-9, 1),
            "distinct_ci": int(np.unique(ci[act]).size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "interception_kernel_resources.txt"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["SMASHX_VERBOSE"] = "1"
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    res = {"what": "smashx_adjust_interception: gr-b, compact forcing built on the device, default build, median of %d calls after one warm-up" % a.reps,
           "device": torch.cuda.get_device_name(0), "sizes": []}
    for n in a.sizes:
        with CapturedStderr():                                 # plan-creation diagnostics of SMASHX_VERBOSE
            r = one_size(n, a.nt, a.reps, torch, dev)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
    probe = os.path.join(ROOT, "profiles", "r2_hbm_probe.json")
    if os.path.exists(probe):
        res["hbm_probe_read_sum_TBps"] = json.load(open(probe))["read_sum_TBps"]
    if os.path.exists(a.resources):
        for line in open(a.resources):
            if line.startswith("sx_k_adjust_interception"):
                res["kernel_resources"] = " ".join(line.split())
    # tests/golden/make_interception.py --time, where the reference lies: its routine alone on the 28 x 28 x 1440 Cance case
    res["reference_one_cpu_core"] = {"case": "gr_a_cance_28x28x1440 (383 active cells x 1440 steps)", "build": "-O2 -ffp-contract=off, best of 5",
                                     "seconds": 0.2124, "cellsteps_per_s": 383 * 1440 / 0.2124,
                                     "note": "timed on one core of the development machine, not on the GPU host"}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
