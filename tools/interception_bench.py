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
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


class CapturedStderr:
    """what the process (the C library included) writes to file descriptor 2 while the block runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def one_size(n, nt, reps, torch, dev):
    import bench
    import smash_amd
    from smash_amd import synth
    from smash_amd.solver import Solver
    t_setup = time.perf_counter()
    m = synth.make_mesh(n, n, ng=1)
    setup = smash_amd.SetupDT(0, 0, structure="gr-b", dt=3600.0, ntime_step=nt)
    mesh = smash_amd.MeshDT(setup, n, n, 0)
    mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.dx, m.flwdir, m.flwacc, m.path, m.active_cell
    mesh.gauge_pos, mesh.area = np.zeros((0, 2), np.int32, order="F"), np.zeros(0, np.float32)
    sol = Solver(setup, mesh)
    sol.set_forcing_layout(compact=True, prcp_factor=0.1, pet_ratio=synth._pet_tables()[1], pet_hour0=0)
    rows, cols = sol.cell_order()
    d_rows = torch.from_numpy(rows.astype(np.int64)).to(dev)
    d_cols = torch.from_numpy(cols.astype(np.int64)).to(dev)
    tb = max(24, (1 << 26) // max(sol.ncells, 1) // 24 * 24)
    for t0 in range(0, nt, tb):
        t1 = min(nt, t0 + tb)
        prcp, pet = bench.forcing_block(d_rows, d_cols, t0, t1, dev)
        torch.cuda.synchronize()
        sol.set_forcing_device_block(t0, t1, prcp.data_ptr(), pet.data_ptr())
        del prcp, pet
    del d_rows, d_cols
    torch.cuda.empty_cache()
    info = sol.forcing_info()
    setup_s = time.perf_counter() - t_setup
    day = (1 + np.arange(nt) // 24).astype(np.int32)          # pet_hour0 = 0: step 0 is hour 0 of day 1
    ci = np.zeros((n, n), np.float32, order="F")
    wall, device, launches = [], [], 0
    for rep in range(reps + 1):                                # the first call is a warm-up (code object load)
        with CapturedStderr() as cap:
            t0 = time.perf_counter()
            sol.adjust_interception(day, ci)
            w = time.perf_counter() - t0
        mt = re.search(r"adjust_interception .*?: ([0-9.]+) ms on the device, (\d+) launches", cap.text)
        if mt is None:
            raise SystemExit("the library did not report its device time (SMASHX_VERBOSE): " + cap.text[-500:])
        if rep:
            wall.append(w); device.append(float(mt.group(1)) * 1e-3); launches = int(mt.group(2))
    cells = sol.ncells
    sol.close()
    act = np.asarray(m.active_cell) == 1
    wall_s, dev_s = statistics.median(wall), statistics.median(device)
    return {"grid": f"{n}x{n}", "cells": cells, "nt": nt, "forcing": info, "setup_s": round(setup_s, 2), "reps": reps,
            "wall_s_median": round(wall_s, 4), "wall_s_all": [round(v, 4) for v in wall],
            "device_s_median": round(dev_s, 4), "device_s_all": [round(v, 4) for v in device], "launches": launches,
            "device_s_per_launch": round(dev_s / launches, 4),
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
