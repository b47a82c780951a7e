#!/usr/bin/env python3
"""Times the signature-based criteria in the cost of the sweeps on the headline grid: gr-b, n^2 cells x 8760 steps, compact forcing
built on the device block by block as bench.py builds it, one outlet gauge plus three nested ones, mean_prcp from smashx_mean_forcing,
a synthetic mask_event (five events per gauge around its wettest steps), observations = a forward run with parameters 10 % off.
Forward and forward + adjoint sweeps with jobs_fun = ("nse",) and with ("nse", "Crc", "Cfp2", "Cfp10", "Cfp50", "Cfp90", "Epf", "Erc"):
median of --reps sweeps after a warm-up, wall time and the device times smashx_get_timing reports from HIP events -- sweep_ms, the
whole sweep, and cost_ms, everything between the first cost kernel and the last (sums, the signature kernels, sx_k_cost_final, the
seeds).  The signature kernels' device time is cost_ms of the eight criteria minus cost_ms of nse alone.

    python tools/signature_cost_bench.py --size 1024 --out profiles/signature_cost_1024.json
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

SET_ALL = ("nse", "Crc", "Cfp2", "Cfp10", "Cfp50", "Cfp90", "Epf", "Erc")


def synthetic_mask(mean_prcp, nt, events=5, before=12, after=60):
    ng = mean_prcp.shape[0]
    mask = np.zeros((ng, nt), np.int32, order="F")
    for g in range(ng):
        picked = []
        for t in np.argsort(-np.nan_to_num(mean_prcp[g], nan=-1.0), kind="stable"):
            if before <= t < nt - after and all(abs(int(t) - q) > before + after for q in picked):
                picked.append(int(t))
            if len(picked) == events:
                break
        for i, t in enumerate(sorted(picked)):
            mask[g, t - before:t + after] = i + 1
    return mask


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--gauges", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "signature_kernel_resources.txt"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import smash_amd
    from smash_amd import synth
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    n, nt, ng = a.size, a.nt, a.gauges
    with CapturedStderr():
        m, mesh, sol, info, setup_s = plan_with_device_forcing(n, nt, ng, torch, dev)
    setup = smash_amd.SetupDT(0, ng, structure="gr-b", dt=3600.0, ntime_step=nt)
    o = setup.optimize
    par = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(n, n))
    sta = smash_amd.StatesDT.from_dict(mesh, synth.make_states(n, n, warm=True))
    parq = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(n, n, perturb=0.1))
    out = smash_amd.OutputDT(setup, mesh)
    o.jobs_fun, o.wjobs_fun = ["nse"], [1.0]
    sol.set_options(o)
    sol.upload(parq, sta)
    sol.sweep(False)
    sol.download(False, parq, sta, out)
    sol.set_qobs(out.qsim)
    mean_prcp, _ = sol.mean_forcing(pet=False)
    o.mask_event = synthetic_mask(mean_prcp, nt)
    sol.set_signature_inputs(mean_prcp, o.mask_event)
    sol.upload(par, sta)
    res = {"what": "signature criteria in the cost: gr-b, compact forcing built on the device, one outlet gauge + %d nested, default build, median of "
                   "%d sweeps after a warm-up; sweep_ms / cost_ms from HIP events (smashx_get_timing)" % (ng - 1, a.reps),
           "device": torch.cuda.get_device_name(0), "grid": f"{n}x{n}", "cells": sol.ncells, "nt": nt, "gauges": ng, "forcing": info,
           "events_per_gauge": [int(o.mask_event[g].max()) for g in range(ng)], "runs": {}}
    for name, jobs in (("nse", ("nse",)), ("eight", SET_ALL)):
        o.jobs_fun, o.wjobs_fun = list(jobs), [1.0 / len(jobs)] * len(jobs)
        sol.set_options(o)
        for adjoint in (False, True):
            sol.sweep(adjoint)
            wall, sweep, cost = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                sol.sweep(adjoint)
                wall.append((time.perf_counter() - t0) * 1e3)
                tm = sol.timing()
                sweep.append(tm["sweep_ms"]); cost.append(tm["cost_ms"])
            res["runs"][f"{name}_{'adjoint' if adjoint else 'forward'}"] = {
                "wall_ms_median": med(wall), "sweep_ms_median": med(sweep), "cost_ms_median": med(cost),
                "sweep_ms_all": [round(v, 3) for v in sweep], "cost_ms_all": [round(v, 3) for v in cost],
                "cost": sol.cost_and_qsim(None)}
            print(name, "adjoint" if adjoint else "forward", res["runs"][f"{name}_{'adjoint' if adjoint else 'forward'}"], flush=True)
    r = res["runs"]
    for k in ("forward", "adjoint"):
        res[f"signature_kernels_ms_{k}"] = round(r[f"eight_{k}"]["cost_ms_median"] - r[f"nse_{k}"]["cost_ms_median"], 4)
        res[f"share_of_the_{k}_sweep"] = round(res[f"signature_kernels_ms_{k}"] / r[f"nse_{k}"]["sweep_ms_median"], 5)
    if os.path.exists(a.resources):
        res["kernel_resources"] = [" ".join(ln.split()) for ln in open(a.resources) if ln.startswith("sx_k_sig")]
    sol.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
