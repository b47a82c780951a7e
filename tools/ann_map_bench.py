#!/usr/bin/env python3
"""Times ONE epoch of the ANN regionalisation (network forward pass over the active cells, forward + adjoint sweep, back-propagation and
weight-gradient sums) on the headline grids: gr-b, n^2 cells x 8760 steps, compact forcing built on the device block by block as
bench.py builds it, nd descriptors, a (32, 16, ncv) relu / relu / sigmoid + scale net on cp, cft, exc, lr, default build, two ways:
  numpy   what the project offered before the device path: a numpy fp64 network around smash_amd.forward_b -- the control fields' planes
          go up and their gradient planes come back over PCIe every epoch
  device  Solver.ann_upload -> sweep -> ann_gradient (include/smashx_ann.h), what ann_optimize(device_map=True) runs; split into map,
          sweep and adjoint map by smashx_ann_info (HIP events) and the sweep's own device time
Per leg the wall time of the epoch, median of --reps after one warm-up.  The two legs' weight gradients are compared (relative L2: numpy
sums in another order and calls another exp).

    python tools/ann_map_bench.py --sizes 1024 2048 --out profiles/ann_map_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hyper_map_bench import median_wall                                     # noqa: E402
from resident_forcing import CapturedStderr, plan_with_device_forcing      # noqa: E402

CONTROL = ("cp", "cft", "exc", "lr")
BOUNDS = ((1.0, 1000.0), (1.0, 1000.0), (-20.0, 5.0), (1.0, 200.0))


def numpy_net(net, x, loss_grad=None):
    """the (dense relu, dense relu, dense sigmoid, scale) net in numpy fp64: outputs, or the packed weight gradient"""
    d = net._dense()
    lo, hi = np.array(BOUNDS).T
    h0 = x.astype(np.float64)
    a1 = h0 @ d[0].weight + d[0].bias
    h1 = np.where(a1 >= 0, a1, 0)
    a2 = h1 @ d[1].weight + d[1].bias
    h2 = np.where(a2 >= 0, a2, 0)
    s = 1 / (1 + np.exp(-(h2 @ d[2].weight + d[2].bias)))
    if loss_grad is None:
        return lo + s * (hi - lo)
    g = loss_grad.astype(np.float64) * (hi - lo) * s * (1 - s)
    out = [h2.T @ g, g.sum(0)]
    g = (g @ d[2].weight.T) * (a2 >= 0)
    out = [h1.T @ g, g.sum(0)] + out
    g = (g @ d[1].weight.T) * (a1 >= 0)
    out = [h0.T @ g, g.sum(0)] + out
    return np.concatenate([o.ravel() for o in out])


def one_size(n, nt, ng, nd, reps, reps_numpy, torch, dev):
    import smash_amd
    from smash_amd import synth
    from smash_amd.solver import STRUCTURE_FIELDS
    m, mesh, sol, finfo, setup_s = plan_with_device_forcing(n, nt, ng, torch, dev)
    rng = np.random.default_rng(11)
    desc = np.asfortranarray(rng.random((n, n, nd), dtype=np.float32))
    qobs = np.asfortranarray((0.2 + 3.0 * rng.random((ng, nt))).astype(np.float32))
    par = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(n, n))
    sta = smash_amd.StatesDT.from_dict(mesh, synth.make_states(n, n, warm=True))
    setup = smash_amd.SetupDT(nd, ng, structure="gr-b", dt=3600.0, ntime_step=nt)
    setup.optimize.jobs_fun, setup.optimize.wjobs_fun = ["nse"], [1.0]
    inp = object.__new__(smash_amd.Input_DataDT)      # no host forcing: the plan holds it (device blocks), forward_b finds the plan on the object
    inp.prcp = inp.pet = inp.sparse_prcp = inp.sparse_pet = None
    inp.qobs, inp.descriptor, inp._smashx_solver = qobs, desc, sol
    sol._sig = sol.signature(setup, mesh)
    net = smash_amd.Net()
    net.add("dense", {"input_shape": (nd,), "neurons": 32})
    net.add("activation", {"name": "relu"})
    net.add("dense", {"neurons": 16})
    net.add("activation", {"name": "relu"})
    net.add("dense", {"neurons": len(CONTROL)})
    net.add("activation", {"name": "sigmoid"})
    net.add("scale", {"bounds": BOUNDS})
    net.compile("adam", random_state=3)
    w = net.weights()
    act = np.asarray(mesh.active_cell) == 1
    cc, rr = np.nonzero(act.T)
    x = np.ascontiguousarray(desc[rr, cc])
    output = smash_amd.OutputDT(setup, mesh)
    sol.set_qobs(qobs)
    sol.set_options(setup.optimize)
    sol.set_ann_descriptors(desc)
    sol.set_ann_net(net, CONTROL)
    sol.upload(par, sta)
    kern, sweep = [], []

    def device():
        sol.ann_upload(w)
        sol.sweep(True, 1.0)
        sol.cost_and_qsim(output)
        g = sol.ann_gradient()
        i = sol.ann_info()
        kern.append((i["map_ms"], i["gradient_ms"]))
        sweep.append(sol.timing()["sweep_ms"])
        return g

    par_b, sta_b = par.copy(), sta.copy()

    def through_numpy():
        y = numpy_net(net, x)
        for i, k in enumerate(CONTROL):
            getattr(par, k)[rr, cc] = y[:, i]
        smash_amd.forward_b(setup, mesh, inp, par, par_b, par, par_b, sta, sta_b, sta, sta_b, output, None, np.float32(0), np.float32(1))
        lg = np.stack([getattr(par_b, k)[rr, cc] for k in CONTROL], axis=1)
        return numpy_net(net, x, lg)

    t_dev, all_dev, g_dev = median_wall(device, reps)
    info = sol.ann_info()
    t_np, all_np, g_np = median_wall(through_numpy, reps_numpy)
    plane = n * n * 4
    nslot = len(STRUCTURE_FIELDS["gr-b"])
    r = {"grid": f"{n}x{n}", "cells": sol.ncells, "nt": nt, "gauges": ng, "nd": nd, "forcing": finfo, "setup_s": round(setup_s, 2),
         "net": {"widths": [32, 16, len(CONTROL)], "weights": int(w.size), "lds_bytes_per_workgroup": info["lds_bytes"], "span_cells": info["span"]},
         "device": {"wall_s_median": round(t_dev, 4), "wall_s_all": all_dev,
                    "map_kernel_ms_median": round(statistics.median(k[0] for k in kern[1:]), 3),
                    "adjoint_map_kernels_ms_median": round(statistics.median(k[1] for k in kern[1:]), 3),
                    "sweep_ms_median": round(statistics.median(sweep[1:]), 2),
                    "pcie_bytes": {"up": int(w.size) * 8, "down": int(w.size) * 8 + ng * nt * 4 + 12}},
         "numpy_around_forward_b": {"wall_s_median": round(t_np, 4), "wall_s_all": all_np, "reps": reps_numpy,
                                    "pcie_bytes": {"up": nslot * plane, "down": nslot * plane + ng * nt * 4 + 12,
                                                   "note": f"{nslot} planes of the fields gr-b reads up and {nslot} gradient planes down, {plane} B each"}},
         "gradient_rel_l2_device_vs_numpy": float(np.linalg.norm(g_dev - g_np) / np.linalg.norm(g_np)),
         "wall_ratio_numpy_over_device": round(t_np / t_dev, 2)}
    d = r["device"]
    d["maps_share_of_sweep"] = round((d["map_kernel_ms_median"] + d["adjoint_map_kernels_ms_median"]) / d["sweep_ms_median"], 4)
    sol.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nt", type=int, default=8760)
    ap.add_argument("--gauges", type=int, default=4)
    ap.add_argument("--nd", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reps-numpy", type=int, default=3, help="repetitions of the numpy leg (tens of seconds each at 2048^2)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    res = {"what": "one epoch of the ANN regionalisation (net forward, forward + adjoint sweep, back-propagation + weight-gradient sums): gr-b, "
                   "compact forcing built on the device, default build, wall time, median of --reps after one warm-up; numpy = a numpy fp64 "
                   "net around smash_amd.forward_b, the path before the device maps",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "sizes": []}
    for n in a.sizes:
        with CapturedStderr():
            r = one_size(n, a.nt, a.gauges, a.nd, a.reps, a.reps_numpy, torch, dev)
        res["sizes"].append(r)
        print(json.dumps(r), flush=True)
        if a.out:                                              # written after every size: a later size that cannot be run loses nothing
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
