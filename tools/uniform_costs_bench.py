"""Measures the three ways to evaluate a batch of spatially uniform candidates on one resident plan -- the catchment-resident kernel
(Solver.uniform_costs), the ensemble (Solver.multiple_run) and the loop of single forwards (smashx_forward per candidate) -- on the
Cance catchment (gr-a, 383 cells x 1440 steps, tests/golden) and on a synthetic 32 x 32 x 8760 gr-b catchment (smash_amd/synth.py), at
S = 1, 8, 64, 256 and 1024 candidates: wall seconds per call, median of --reps calls after one warm-up, the download of the costs
included, and the device time of the resident and ensemble calls (HIP events).  Then the wall time of smash_amd.optimize_sbs on Cance
(cp, cft, exc, lr from the Model() defaults, --maxiter iterations) per route.  One JSON line (also written to --out).

    python tools/uniform_costs_bench.py --out profiles/uniform_costs.json [--only cance --samples 8 --reps 5 --maxiter 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import smash_amd                                             # noqa: E402
from smash_amd import _lib, synth                            # noqa: E402
from smash_amd.solver import FIELD_NAMES, PARAM_NAMES, STATE_NAMES, STRUCTURE_FIELDS, Solver, _pack_const   # noqa: E402
from ensemble_bench import draw, median                      # noqa: E402


def cases(only):
    out = []
    if only in (None, "cance"):
        import golden_util as gu
        g = gu.load("gr_a_cance_28x28x1440")
        out.append(("cance_gr_a_383x1440", g.structure, g.mesh, g.dt, g.nt, g.prcp, g.pet, g.qobs, g.params, g.states, g.opts.get("wgauge")))
    if only in (None, "synth"):
        m = synth.make_mesh(32, 32, ng=4)
        nt = 8760
        prcp, pet = synth.dense_forcing(m, nt)
        qobs = np.asfortranarray(np.random.default_rng(1).uniform(0.1, 5.0, (m.ng, nt)).astype(np.float32))
        out.append(("synth_gr_b_1024x8760", "gr-b", m, 3600.0, nt, prcp, pet, qobs, synth.make_parameters(32, 32), synth.make_states(32, 32, warm=True), None))
    return out


def sbs_on_cance(maxiter):
    """the user guide's first calibration per route: wall seconds of the whole call, the trajectory's length and end"""
    import golden_util as gu
    g = gu.load("gr_a_cance_28x28x1440")
    pv = dict(ci=1e-6, cp=200.0, beta=1000.0, cft=500.0, cst=500.0, alpha=0.9, exc=0.0, lr=5.0)
    out = {}
    for route in ("resident", "ensemble", "loop", "auto"):
        setup = smash_amd.SetupDT(0, g.mesh.ng, structure=g.structure, dt=g.dt, ntime_step=g.nt)
        o = setup.optimize
        o.jobs_fun, o.wjobs_fun, o.maxiter = ["nse"], [1.0], maxiter
        if "wgauge" in g.opts:
            o.wgauge = np.asarray(g.opts["wgauge"], np.float32)
        o.optim_parameters = np.array([1 if k in ("cp", "cft", "exc", "lr") else 0 for k in PARAM_NAMES], np.int32)
        o.optim_states = np.zeros(8, np.int32)
        mesh = smash_amd.MeshDT.from_synth(setup, g.mesh)
        inp = smash_amd.Input_DataDT(setup, mesh)
        inp.prcp, inp.pet, inp.qobs = g.prcp, g.pet, g.qobs
        times = []
        for rep in range(2):         # the first call builds the plan and uploads the forcing
            par = smash_amd.ParametersDT.from_dict(mesh, {k: (np.full_like(v, pv[k]) if k in pv else v) for k, v in g.params.items()})
            sta = smash_amd.StatesDT.from_dict(mesh, g.states)
            t = time.perf_counter()
            h = smash_amd.optimize_sbs(setup, mesh, inp, par, sta, smash_amd.OutputDT(setup, mesh), candidates=route)
            times.append(time.perf_counter() - t)
        out[route] = {"seconds_first_call": times[0], "seconds": times[1], "nfg": h["nfg_total"], "inner_iterations": h["iter"],
                      "final_cost": h["final_cost"], "task": h["task"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("cance", "synth"), default=None)
    ap.add_argument("--samples", type=int, nargs="*", default=[1, 8, 64, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=10)
    a = ap.parse_args()
    res = {"tool": "tools/uniform_costs_bench.py", "exact_libm": bool(_lib.EXACT), "reps": a.reps, "cases": {}}
    L = _lib.lib()
    for name, structure, m, dt, nt, prcp, pet, qobs, params, states, wgauge in cases(a.only):
        setup = smash_amd.SetupDT(0, m.ng, structure=structure, dt=dt, ntime_step=nt)
        setup.optimize.jobs_fun, setup.optimize.wjobs_fun = ["nse"], [1.0]
        if wgauge is not None:
            setup.optimize.wgauge = np.asarray(wgauge, np.float32)
        mesh = smash_amd.MeshDT.from_synth(setup, m)
        par, sta = smash_amd.ParametersDT.from_dict(mesh, params), smash_amd.StatesDT.from_dict(mesh, states)
        s = Solver(setup, mesh)
        s.set_forcing(prcp, pet)
        s.set_qobs(qobs)
        s.set_options(setup.optimize)
        names = [k for k in STRUCTURE_FIELDS[structure] if k in PARAM_NAMES] + [k for k in STRUCTURE_FIELDS[structure] if k in STATE_NAMES][:2]
        ind = np.array([FIELD_NAMES.index(k) + 1 for k in names], np.int32)
        case = {"cells": s.ncells, "steps": nt, "gauges": m.ng, "sampled_fields": names, "resident": {}, "ensemble": {}, "loop": {}}
        p, st_ = par.copy(), sta.copy()
        P, k1 = _pack_const(p, PARAM_NAMES, _lib.Parameters)
        St, k2 = _pack_const(st_, STATE_NAMES, _lib.States)
        qs = np.zeros((m.ng, nt), np.float32, order="F")
        costs = _lib.Costs()
        for S in a.samples:
            sample = draw(names, S)
            rc, ec, lc = np.zeros(S, np.float32), np.zeros(S, np.float32), np.zeros(S, np.float32)

            def resident():
                t = time.perf_counter()
                s.uniform_costs(par, sta, sample, ind, res_cost=rc)
                return time.perf_counter() - t, s.uniform_costs_info()["device_ms"] * 1e-3

            def ensemble():
                t = time.perf_counter()
                s.multiple_run(par, sta, sample, ind, res_cost=ec)
                return time.perf_counter() - t, s.multiple_run_info()["device_ms"] * 1e-3

            def loop():
                t = time.perf_counter()
                for i in range(S):
                    for k, v in zip(names, sample[:, i]):
                        getattr(p if k in PARAM_NAMES else st_, k)[...] = v
                    _lib.check(L.smashx_forward(s._h, C.byref(P), C.byref(P), C.byref(St), C.byref(St), qs.ctypes.data_as(C.c_void_p), C.byref(costs), None))
                    lc[i] = costs.cost
                return time.perf_counter() - t, 0.0
            for key, fn in (("resident", resident), ("ensemble", ensemble), ("loop", loop)):
                fn()             # warm-up
                runs = [fn() for _ in range(a.reps)]
                case[key][str(S)] = {"seconds_per_call": median([r[0] for r in runs]), "wall_min_max": [min(r[0] for r in runs), max(r[0] for r in runs)]}
                if key != "loop":
                    case[key][str(S)]["device_seconds"] = median([r[1] for r in runs])
            same = lambda x, y: bool(np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32)))
            case["resident"][str(S)]["equals_the_loop_bit_for_bit"] = same(rc, lc)
            case["ensemble"][str(S)]["equals_the_loop_bit_for_bit"] = same(ec, lc)
        case["resident_info"] = s.uniform_costs_info()
        sec = lambda key, S: case[key][str(S)]["seconds_per_call"]
        case["fastest_route"] = {str(S): min(("resident", "ensemble", "loop"), key=lambda k: sec(k, S)) for S in a.samples}
        over = [S for S in a.samples if sec("ensemble", S) < sec("resident", S)]
        case["ensemble_overtakes_resident_at_S"] = over[0] if over else None
        res["cases"][name] = case
        s.close()
    if a.only in (None, "cance") and a.maxiter > 0:
        res["optimize_sbs_cance"] = dict(maxiter=a.maxiter, routes=sbs_on_cance(a.maxiter))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
