#!/usr/bin/env python3
"""Times ONE evaluation of the regionalisation's cost and gradient (base_hyper_forward_b: map, forward + adjoint sweep, adjoint of the
map) on the headline grids: gr-b, n^2 cells x 8760 steps, compact forcing built on the device block by block as bench.py builds it,
hyper-linear and hyper-polynomial with nd descriptors, default build, with the maps
  on   the device: Solver.hyper_upload -> sweep -> hyper_gradient (include/smashx_hyper.h), what optimize_hyper_lbfgsb(device_map=True) runs
  off  the host:   smash_amd.hyper_forward_b, the composition of sx_hyper.cpp's maps with smashx_upload / smashx_download, unchanged by
                   the device maps: the baseline
Per leg: wall time of the evaluation, median of --reps after one warm-up; for the device leg also the two kernels' own times (HIP events,
smashx_hyper_info), the sweep's device time, and for both the bytes an evaluation moves across PCIe (counted from the calls' arguments:
planes of the fields the structure reads, matrices, the discharge).  The two legs' gradients are compared bit for bit.

    python tools/hyper_map_bench.py --sizes 1024 2048 --out profiles/hyper_device_map.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from resident_forcing import CapturedStderr, plan_with_device_forcing      # noqa: E402


def median_wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(t, 4) for t in ts], r


def one_size(n, nt, ng, nd, reps, reps_off, torch, dev):
    import smash_amd
    from smash_amd import synth
    from smash_amd.optimize import hyper_problem_initialise
    from smash_amd.solver import STRUCTURE_FIELDS
    m, mesh, sol, finfo, setup_s = plan_with_device_forcing(n, nt, ng, torch, dev)
    rng = np.random.default_rng(11)
    desc = np.asfortranarray(rng.random((n, n, nd), dtype=np.float32))
    desc[0, 0, :], desc[1, 0, :] = 0.0, 1.0
    qobs = np.asfortranarray((0.2 + 3.0 * rng.random((ng, nt))).astype(np.float32))
    par0 = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(n, n))
    sta0 = smash_amd.StatesDT.from_dict(mesh, synth.make_states(n, n, warm=True))
    out = {"grid": f"{n}x{n}", "cells": sol.ncells, "nt": nt, "gauges": ng, "nd": nd, "forcing": finfo, "setup_s": round(setup_s, 2), "mappings": {}}
    nslot = len(STRUCTURE_FIELDS["gr-b"])
    for mapping in ("hyper-linear", "hyper-polynomial"):
        setup = smash_amd.SetupDT(nd, ng, structure="gr-b", dt=3600.0, ntime_step=nt)
        o = setup.optimize
        o.mapping, o.nhyper, o.jobs_fun, o.wjobs_fun = mapping, 1 + nd * (2 if mapping == "hyper-polynomial" else 1), ["nse"], [1.0]
        # an input_data without host forcing: the plan holds it (device blocks), the host composition finds the plan on the object
        inp = object.__new__(smash_amd.Input_DataDT)
        inp.prcp = inp.pet = inp.sparse_prcp = inp.sparse_pet = None
        inp.qobs, inp.descriptor, inp._smashx_solver = qobs, desc, sol
        sol._sig = sol.signature(setup, mesh)
        HP, HS, *_ = hyper_problem_initialise(setup, mesh, par0, sta0)
        M = HP.matrix()
        if mapping == "hyper-polynomial":
            M[1::2], M[2::2] = 0.1, 1.3
        else:
            M[1:] = 0.1
        HP.set_matrix(M)
        hpm, hsm = HP.matrix(), HS.matrix()
        output = smash_amd.OutputDT(setup, mesh)
        sol.set_qobs(qobs)
        sol.set_options(setup.optimize)
        sol.set_hyper_descriptors(mapping, desc)
        kern, sweep = [], []

        def on():
            sol.hyper_upload(hpm, hsm)
            sol.sweep(True, 1.0)
            sol.cost_and_qsim(output)
            g = sol.hyper_gradient()
            i = sol.hyper_info()
            kern.append((i["map_ms"], i["gradient_ms"]))
            sweep.append(sol.timing()["sweep_ms"])
            return g

        par, sta = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
        par_b, sta_b = par.copy(), sta.copy()

        def off():
            HPb, HSb = HP.copy(), HS.copy()
            smash_amd.hyper_forward_b(setup, mesh, inp, par, par_b, HP, HPb, HP, sta, sta_b, HS, HSb, HS, output, None, np.float32(0), np.float32(1))
            return HPb.matrix(), HSb.matrix()

        t_on, all_on, g_on = median_wall(on, reps)
        info = sol.hyper_info()
        t_off, all_off, g_off = median_wall(off, reps_off)
        nh = o.nhyper
        plane = n * n * 4
        r = {"nhyper": nh, "chains": info["chains"], "span_cells": info["span"],
             "device_map_on": {"wall_s_median": round(t_on, 4), "wall_s_all": all_on,
                               "map_kernel_ms_median": round(statistics.median(k[0] for k in kern[1:]), 3),
                               "gradient_kernels_ms_median": round(statistics.median(k[1] for k in kern[1:]), 3),
                               "sweep_ms_median": round(statistics.median(sweep[1:]), 2),
                               "pcie_bytes": {"up": 24 * nh * 4, "down": 24 * nh * 4 + ng * nt * 4 + 12}},
             "device_map_off": {"wall_s_median": round(t_off, 4), "wall_s_all": all_off, "reps": reps_off,
                                "pcie_bytes": {"up": nslot * plane, "down": nslot * plane + ng * nt * 4 + 12,
                                               "note": f"{nslot} planes of the fields gr-b reads up and {nslot} gradient planes down, {plane} B each"}},
             "gradients_bit_equal": bool(all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(g_on, g_off))),
             "wall_ratio_off_over_on": round(t_off / t_on, 2)}
        r["device_map_on"]["maps_share_of_sweep"] = round((r["device_map_on"]["map_kernel_ms_median"] + r["device_map_on"]["gradient_kernels_ms_median"])
                                                          / r["device_map_on"]["sweep_ms_median"], 4)
        out["mappings"][mapping] = r
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--gauges", type=int, default=4)
    ap.add_argument("--nd", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-off", type=int, default=5, help="repetitions of the host leg (tens of seconds each at 2048^2)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    res = {"what": "one evaluation of cost + gradient of the hyper maps (map, forward + adjoint sweep, adjoint of the map): gr-b, compact forcing "
                   "built on the device, default build, wall time, median of --reps after one warm-up; device_map off = smash_amd.hyper_forward_b, "
                   "the path before the device maps",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "sizes": []}
    for n in a.sizes:
        with CapturedStderr():
            r = one_size(n, a.nt, a.gauges, a.nd, a.reps, a.reps_off, torch, dev)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
        if a.out:                                              # written after every size: a later size that cannot be run loses nothing
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
