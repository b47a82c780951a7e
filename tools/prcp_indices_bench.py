#!/usr/bin/env python3
"""Times smashx_prcp_indices (compute_prcp_indices on the resident rain) beside smashx_mean_forcing (rain only) IN THE SAME RUN on the
headline grids: gr-b, n^2 cells x 8760 steps, compact forcing built on the device block by block as bench.py builds it, one outlet
gauge plus three nested ones (the gauges of tools/mean_forcing_bench.py), default build.  Per size and call: wall time and the device
time between the first and last launch (HIP events around the launches; the library prints it under SMASHX_VERBOSE and the call's
stderr is captured), median of --reps after one warm-up, the ratio of the two passes beside the ratio of their list entries
((catchment + bin entries) / catchment entries), and the two floors of DESIGN.md 9e:
  bytes   the resident rain of every list entry (catchments and bins), read once, at the read rate tools/hbm_probe.py sustains
  chain   the longest list: one dependent fp32 addition per entry (CHAIN_CYCLES_PER_CELL cycles at CLOCK_GHZ)

    python tools/prcp_indices_bench.py --sizes 1024 2048 --out profiles/prcp_indices_1024_2048.json
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
RAIN_BYTES = 2.0                 # the compact layout holds the rain as one u16 per cell-step


def one_size(n, nt, ng, reps, torch, dev, hbm_TBps):
    m, mesh, sol, info, setup_s = plan_with_device_forcing(n, nt, ng, torch, dev)
    flwdst = mesh.flwdst
    catch = [int(m.flwacc[r, c]) for r, c in np.asarray(m.gauge_pos).reshape(-1, 2)]
    mp = np.zeros((ng, nt), np.float32, order="F")
    out = np.full((4, ng, nt), -1.0, np.float32, order="F")
    mean, _ = timed(lambda: sol.mean_forcing(mp, None, pet=False), r"mean_forcing .*?: (?P<ms>[0-9.]+) ms on the device, (?P<launches>\d+) launches", reps)
    pi, mt = timed(lambda: sol.prcp_indices(flwdst, out),
                   r"prcp_indices .*?longest list (?P<blocks>\d+) blocks, (?P<entries>\d+) list entries \((?P<catch>\d+) of catchments\), (?P<written>\d+) pairs written: "
                   r"(?P<ms>[0-9.]+) ms on the device, (?P<launches>\d+) launches", reps)
    cells = sol.ncells
    sol.close()
    entries, centries, longest = int(mt.group("entries")), int(mt.group("catch")), int(mt.group("blocks")) * 64
    assert centries == sum(catch)
    return {"grid": f"{n}x{n}", "cells": cells, "nt": nt, "gauges": ng, "catchment_cells": catch, "forcing": info, "setup_s": round(setup_s, 2), "reps": reps,
            "mean_forcing_prcp_only": mean, "prcp_indices": pi,
            "list_entries_padded": entries, "catchment_entries": centries, "longest_list_entries": longest, "pairs_written": int(mt.group("written")),
            "ratio_device_time": round(pi["device_s_median"] / mean["device_s_median"], 3),
            "ratio_list_entries": round(entries / centries, 3),
            "ns_per_entry_of_the_longest_list": round(pi["device_s_median"] / longest * 1e9, 2),
            "floor_bytes_s": round(float(entries) * nt * RAIN_BYTES / (hbm_TBps * 1e12), 4),
            "floor_chain_s": round(longest * CHAIN_CYCLES_PER_CELL / (CLOCK_GHZ * 1e9), 4),
            "gathered_GBps": round(float(entries) * nt * RAIN_BYTES / pi["device_s_median"] * 1e-9, 1),
            "finite_entries": int(np.isfinite(out).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--gauges", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "prcp_indices_kernel_resources.txt"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["SMASHX_VERBOSE"] = "1"
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    hbm = json.load(open(os.path.join(ROOT, "profiles", "r2_hbm_probe.json")))["read_sum_TBps"]
    res = {"what": "smashx_prcp_indices beside smashx_mean_forcing (rain only) in the same run: gr-b, compact forcing built on the device, one outlet gauge + %d "
                   "nested, default build, median of %d calls after one warm-up, device time from HIP events around the launches" % (a.gauges - 1, a.reps),
           "device": torch.cuda.get_device_name(0), "hbm_probe_read_sum_TBps": hbm,
           "chain_floor_assumes": f"{CHAIN_CYCLES_PER_CELL} cycles per entry of the longest list at {CLOCK_GHZ} GHz", "sizes": []}
    for n in a.sizes:
        with CapturedStderr():                                 # plan-creation diagnostics of SMASHX_VERBOSE
            r = one_size(n, a.nt, a.gauges, a.reps, torch, dev, hbm)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
        if a.out:                                              # written after every size: a later size that cannot be run loses nothing
            if os.path.exists(a.resources):
                res["kernel_resources"] = [" ".join(line.split()) for line in open(a.resources) if "sx_k_prcp_indices" in line]
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
