#!/usr/bin/env python3
"""Times smashx_mean_forcing (compute_mean_forcing on the resident forcing) on the headline grids: gr-b, n^2 cells x 8760 steps,
compact forcing built on the device block by block as bench.py builds it, one outlet gauge plus three nested ones, default build.
Per size: wall time of the call and the device time between its first and last launch (HIP events around the launches; the library
prints it under SMASHX_VERBOSE and the call's stderr is captured), median of --reps after one warm-up, beside the two floors of
DESIGN.md 9d:
  bytes   the resident forcing of the cells each gauge sums over, read once per gauge (and: of every cell once), at the read rate
          tools/hbm_probe.py sustains (profiles/r2_hbm_probe.json)
  chain   the longest catchment list x one dependent fp32 addition per cell (CHAIN_CYCLES_PER_CELL cycles at CLOCK_GHZ): what a single
          lane's sum costs when every value is already there; only ng * ceil(nt / 64) wavefronts exist to hide anything else
and the kernel's registers, waves per SIMD and LDS (a listing written by tools/kernel_resources.py).

    python tools/mean_forcing_bench.py --sizes 1024 2048 --out profiles/mean_forcing_1024_2048.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from resident_forcing import CapturedStderr, plan_with_device_forcing, timed      # noqa: E402

CHAIN_CYCLES_PER_CELL = 4.0      # a dependent VALU instruction of one wavefront: 64 lanes over a 16-wide SIMD
CLOCK_GHZ = 2.4


def one_size(n, nt, ng, reps, torch, dev, hbm_TBps):
    m, _, sol, info, setup_s = plan_with_device_forcing(n, nt, ng, torch, dev)
    catch = [int(m.flwacc[r, c]) for r, c in np.asarray(m.gauge_pos).reshape(-1, 2)]     # cells upstream of a gauge, itself included
    mp = np.zeros((ng, nt), np.float32, order="F")
    me = np.zeros((ng, nt), np.float32, order="F")
    t, _ = timed(lambda: sol.mean_forcing(mp, me), r"mean_forcing .*?: (?P<ms>[0-9.]+) ms on the device, (?P<launches>\d+) launches", reps)
    cells = sol.ncells
    sol.close()
    dev_s = t["device_s_median"]
    bpc = info["resident_bytes_per_cellstep"]
    gathered = float(sum(catch)) * nt * bpc
    once = float(cells) * nt * bpc
    chain_s = max(catch) * CHAIN_CYCLES_PER_CELL / (CLOCK_GHZ * 1e9)
    return {"grid": f"{n}x{n}", "cells": cells, "nt": nt, "gauges": ng, "catchment_cells": catch, "forcing": info, "setup_s": round(setup_s, 2),
            "reps": reps, **t, "device_s_per_launch": round(dev_s / t["launches"], 4), "wavefronts_of_steps": ng * ((nt + 63) // 64),
            "masked_cellsteps_per_s_device": float(sum(catch)) * nt / dev_s,
            "ns_per_cell_of_the_longest_list": round(dev_s / max(catch) * 1e9, 2),
            "floor_bytes_s": {"every_gauge_reads_its_cells": round(gathered / (hbm_TBps * 1e12), 4), "every_cell_once": round(once / (hbm_TBps * 1e12), 4)},
            "floor_chain_s": round(chain_s, 4),
            "gathered_GBps": round(gathered / dev_s * 1e-9, 1),
            "finite_means": int(np.isfinite(mp).sum() + np.isfinite(me).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--gauges", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "mean_forcing_kernel_resources.txt"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["SMASHX_VERBOSE"] = "1"
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    hbm = json.load(open(os.path.join(ROOT, "profiles", "r2_hbm_probe.json")))["read_sum_TBps"]
    res = {"what": "smashx_mean_forcing: gr-b, compact forcing built on the device, one outlet gauge + %d nested, default build, median of %d calls "
                   "after one warm-up, device time from HIP events around the launches" % (a.gauges - 1, a.reps),
           "device": torch.cuda.get_device_name(0), "hbm_probe_read_sum_TBps": hbm,
           "chain_floor_assumes": f"{CHAIN_CYCLES_PER_CELL} cycles per cell of the longest list at {CLOCK_GHZ} GHz", "sizes": []}
    for n in a.sizes:
        with CapturedStderr():                                 # plan-creation diagnostics of SMASHX_VERBOSE
            r = one_size(n, a.nt, a.gauges, a.reps, torch, dev, hbm)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
        if a.out:                                              # written after every size: a later size that cannot be run loses nothing
            if os.path.exists(a.resources):
                for line in open(a.resources):
                    if line.startswith("sx_k_mean_forcing"):
                        res["kernel_resources"] = " ".join(line.split())
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
