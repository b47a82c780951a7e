"""Measures the ensemble path (smash_amd.Solver.multiple_run) against the loop of single forward runs it replaces: the Cance
catchment (gr-a, 383 cells x 1440 steps, tests/golden) and a synthetic 64 x 64 x 8760 gr-b catchment (smash_amd/synth.py), at
S = 64, 1024 and 16384 samples.  One JSON line (also written to --out).

Per case and S: wall seconds per call (median of --reps after one warm-up, the download of res_cost included), device time of
the call (HIP events), cell-timesteps/s, the batch size and time chunk the library chose, and the achieved rate of the 16 B per
cell-step-sample the design moves (qt written and read, q written and read once by its downstream cell).  The loop is timed at
S = 64 and 1024 (smashx_forward per sample on the same resident plan); above that it is extrapolated per sample and labelled so.

    python tools/ensemble_bench.py --out profiles/ensemble_cance_and_synth.json [--only cance --samples 16384 --reps 1]
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

import smash_amd                                             # noqa: E402
from smash_amd import _lib, synth, types                     # noqa: E402
from smash_amd.solver import FIELD_NAMES, PARAM_NAMES, STATE_NAMES, STRUCTURE_FIELDS, Solver, _pack_const   # noqa: E402


def cases(only):
    out = []
    if only in (None, "cance"):
        import golden_util as gu
        g = gu.load("gr_a_cance_28x28x1440")
        out.append(("cance_gr_a_383x1440", g.structure, g.mesh, g.dt, g.nt, g.prcp, g.pet, g.qobs, g.params, g.states,
                    g.opts.get("wgauge")))
    if only in (None, "synth"):
        m = synth.make_mesh(64, 64, ng=4)
        nt = 8760
        prcp, pet = synth.dense_forcing(m, nt)
        rng = np.random.default_rng(1)
        qobs = np.asfortranarray(rng.uniform(0.1, 5.0, (m.ng, nt)).astype(np.float32))
        out.append(("synth_gr_b_4096x8760", "gr-b", m, 3600.0, nt, prcp, pet, qobs, synth.make_parameters(64, 64),
                    synth.make_states(64, 64, warm=True), None))
    return out


def draw(names, S, seed=4):
    u = np.random.default_rng(seed).random((S, len(names)))
    out = np.zeros((len(names), S), np.float32, order="F")
    for j, k in enumerate(names):
        i = FIELD_NAMES.index(k)
        lo, hi = (types.GLB_PARAMETERS[i], types.GUB_PARAMETERS[i]) if i < 16 else (types.GLB_STATES[i - 16], types.GUB_STATES[i - 16])
        out[j, :] = (lo + (hi - lo) * u[:, j]).astype(np.float32)
    return out


def median(v):
    return float(sorted(v)[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("cance", "synth"), default=None)
    ap.add_argument("--samples", type=int, nargs="*", default=[64, 1024, 16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    res = {"tool": "tools/ensemble_bench.py", "exact_libm": bool(_lib.EXACT), "reps": a.reps, "bytes_per_cellstep_sample_by_design": 16,
           "cases": {}}
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
        ncells = s.ncells
        names = [k for k in STRUCTURE_FIELDS[structure] if k in PARAM_NAMES] + [k for k in STRUCTURE_FIELDS[structure] if k in STATE_NAMES][:2]
        ind = np.array([FIELD_NAMES.index(k) + 1 for k in names], np.int32)
        case = {"cells": ncells, "steps": nt, "gauges": m.ng, "sampled_fields": names, "ensemble": {}, "loop": {}}
        per_forward = None
        for S in a.samples:
            sample = draw(names, S)
            rc = np.zeros(S, np.float32)
            s.multiple_run(par, sta, sample, ind, res_cost=rc)        # warm-up (allocates the buffers)
            wall, dev = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                s.multiple_run(par, sta, sample, ind, res_cost=rc)
                wall.append(time.perf_counter() - t)
                dev.append(s.multiple_run_info()["device_ms"] * 1e-3)
            info = s.multiple_run_info()
            w, d = median(wall), median(dev)
            work = float(ncells) * nt * S
            case["ensemble"][str(S)] = {"seconds_per_call": w, "device_seconds": d, "wall_min_max": [min(wall), max(wall)],
                                        "cellsteps_per_s": work / w, "batch": info["batch"], "chunk": info["chunk"],
                                        "n_batches": info["n_batches"], "n_chunks": info["n_chunks"],
                                        "achieved_GB_per_s_of_the_16_B": 16.0 * work / d / 1e9, "finite_costs": int(np.isfinite(rc).sum())}
            if a.no_loop:
                continue
            if S <= 1024:
                p, st_ = par.copy(), sta.copy()
                P, k1 = _pack_const(p, PARAM_NAMES, _lib.Parameters)
                St, k2 = _pack_const(st_, STATE_NAMES, _lib.States)
                qs = np.zeros((m.ng, nt), np.float32, order="F")
                costs = _lib.Costs()
                L = _lib.lib()

                def loop():
                    t = time.perf_counter()
                    for i in range(S):
                        for k, v in zip(names, sample[:, i]):
                            getattr(p if k in PARAM_NAMES else st_, k)[...] = v
                        _lib.check(L.smashx_forward(s._h, C.byref(P), C.byref(P), C.byref(St), C.byref(St), qs.ctypes.data_as(C.c_void_p),
                                                    C.byref(costs), None))
                    return time.perf_counter() - t
                if S <= 64:
                    loop()      # warm-up
                tl = median([loop() for _ in range(3 if S <= 64 else 1)])
                per_forward = tl / S
                case["loop"][str(S)] = {"seconds": tl, "cellsteps_per_s": work / tl, "measured": True, "speedup_of_the_ensemble": tl / w}
            elif per_forward is not None:
                case["loop"][str(S)] = {"seconds": per_forward * S, "cellsteps_per_s": work / (per_forward * S), "measured": False,
                                        "note": "extrapolated per sample from the largest measured loop", "speedup_of_the_ensemble": per_forward * S / w}
        res["cases"][name] = case
        s.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
