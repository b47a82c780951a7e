"""Variational calibration loop on the host: the mirror of mw_optimize::optimize_lbfgsb
(smash/solver/optimize/mw_optimize.f90:484-676) over GPU sweeps.

Same steps as the reference: normalise the control (mwd_parameters_manipulation.f90:154-178), background = normalised
start, control vector = optimised fields x active cells in column-major order (var_to_control_lbfgsb :679-718, fp32 ->
fp64), L-BFGS-B with m = 10, factr = 10, pgtol = 1e-12 and bounds [0, 1] (:505-512, 541-543), every function/gradient
evaluation one forward_b with denormalize_forward on (:590-606), the two extra stop tests (:625-633), a final forward
(:646-647).  The L-BFGS-B driver is the library's own (smashx_lbfgsb_*, written from the papers the reference's lbfgsb.f
implements; round 3) -- scipy's build of that very code is one environment variable away (SMASHX_LBFGSB=scipy) and, fed by
the CPU oracle, reproduces the reference's cost trajectory bit for bit (tests/test_oracle_golden.py); the native driver
follows it to rounding of the inner products.
"""
from __future__ import annotations

import numpy as np

from .solver import _solver_for, forward
from .synth import PARAM_NAMES, STATE_NAMES


def _normalize(obj, names, lb, ub):
    for i, k in enumerate(names):
        a = getattr(obj, k)
        setattr(obj, k, np.asfortranarray(((a - np.float32(lb[i])) / (np.float32(ub[i]) - np.float32(lb[i]))).astype(np.float32)))


class _Held:
    """a trial point a worker rank has already received (Decomposition.bcast_point hands it back unchanged)"""

    def __init__(self, x):
        self.x = x


class _Stop(Exception):
    pass


def _lbfgsb_native(fg, x0, m, factr, pgtol, maxiter, maxfun, callback, lower=None, upper=None):
    """The library's own L-BFGS-B (include/smashx.h smashx_lbfgsb_*: written from Byrd-Lu-Nocedal-Zhu 1995 / Morales-Nocedal 2011 /
    More'-Thuente, threaded host C++) on the box [0, 1]^n.  No scipy in the loop.  Same method, parameters and stopping tests as the
    lbfgsb.f the reference calls; on test problems its iterates agree with scipy's build of that code to 1e-15 per iteration
    (tests/test_cabi_cpu.py).  lower / upper: other bounds than the box (+-inf = none on that side).  Returns (x, f, info) like
    _lbfgsb_scipy."""
    import ctypes as C
    from . import _lib
    L = _lib.lib()
    n = x0.size
    lo = np.zeros(n, np.float64) if lower is None else np.ascontiguousarray(lower, np.float64)
    up = np.ones(n, np.float64) if upper is None else np.ascontiguousarray(upper, np.float64)
    h = C.c_void_p()
    _lib.check(L.smashx_lbfgsb_create(n, m, lo.ctypes.data, up.ctypes.data, factr, pgtol, C.byref(h)))
    try:
        x = np.array(x0, dtype=np.float64)
        task, f, g = C.c_int(_lib.LBFGSB_START), 0.0, np.zeros(n, np.float64)
        nit = nfev = 0
        stop = None
        while True:
            _lib.check(L.smashx_lbfgsb_step(h, x.ctypes.data, f, g.ctypes.data, C.byref(task)))
            if task.value == _lib.LBFGSB_FG:                # f and g wanted at x
                # (x itself, not a copy: fg reads it before it returns and the optimiser only moves it in its next step -- 134 MB
                # per evaluation at 1.7e7 variables)
                f, g = fg(x)
                g = np.ascontiguousarray(g, np.float64)
                nfev += 1
            elif task.value == _lib.LBFGSB_NEW_X:           # new iterate
                nit += 1
                if callback is not None:
                    if getattr(callback, "wants_pg", False):
                        # the optimiser's own |projected gradient| at this iterate (lbfgsb.f dsave(13)) saves the callback five passes
                        # over x; such a callback copies x itself if it keeps it
                        callback(x, L.smashx_lbfgsb_projected_gradient(h))
                    else:
                        callback(np.copy(x))
                if nit >= maxiter:
                    stop = "STOP: TOTAL NO. of ITERATIONS REACHED LIMIT"
                    break
                if nfev > maxfun:
                    stop = "STOP: TOTAL NO. of f AND g EVALUATIONS EXCEEDS LIMIT"
                    break
            else:
                break
        msg = stop or L.smashx_lbfgsb_message(h).decode()
        return x, float(f), {"task": msg, "nit": nit, "funcalls": nfev, "grad": g}
    finally:
        L.smashx_lbfgsb_destroy(h)


def _lbfgsb_scipy(fg, x0, m, factr, pgtol, maxiter, maxfun, callback):
    """scipy's build of the Zhu-Byrd-Lu-Nocedal 3.0 code the reference carries as lbfgsb.f, for comparison (SMASHX_LBFGSB=scipy):
    bit-identical iterates to the reference's.  scipy's public drivers walk the bounds in Python loops over n before they start --
    tens of seconds for the 1.7e7 control variables of a 2048 x 2048 grid -- so where its `setulb` entry point has the signature of
    scipy 1.15 the driver loop (scipy/optimize/_lbfgsb_py.py::_minimize_lbfgsb) is restated around it with the bound arrays built in
    one go; any other scipy goes through the public fmin_l_bfgs_b.  Returns (x, f, info)."""
    import scipy
    from scipy.optimize import fmin_l_bfgs_b
    n = x0.size
    try:
        from scipy.optimize import _lbfgsb
        direct = tuple(int(v) for v in scipy.__version__.split(".")[:2]) == (1, 15) and hasattr(_lbfgsb, "setulb")
    except Exception:  # pragma: no cover
        direct = False
    if not direct:  # pragma: no cover
        return fmin_l_bfgs_b(fg, x0, m=m, factr=factr, pgtol=pgtol, bounds=[(0.0, 1.0)] * n, maxiter=maxiter, maxfun=maxfun,
                             callback=callback)
    x = np.clip(np.array(x0, dtype=np.float64), 0.0, 1.0)
    nbd = np.full(n, 2, np.int32)                       # both bounds present
    low, up = np.zeros(n, np.float64), np.ones(n, np.float64)
    f = np.array(0.0, dtype=np.int32)                   # (scipy's own driver starts from this placeholder; setulb never reads it before task 3)
    g = np.zeros(n, np.float64)
    wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
    iwa = np.zeros(3 * n, np.int32)
    task, ln_task, lsave = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(4, np.int32)
    isave, dsave = np.zeros(44, np.int32), np.zeros(29, np.float64)
    nit = nfev = 0
    while True:
        g = np.asarray(g, np.float64)
        _lbfgsb.setulb(m, x, low, up, nbd, f, g, factr, pgtol, wa, iwa, task, lsave, isave, dsave, 20, ln_task)
        if task[0] == 3:                                # f and g wanted at x
            f, g = fg(np.copy(x))
            nfev += 1
        elif task[0] == 1:                              # new iterate
            nit += 1
            if callback is not None:
                callback(np.copy(x))
            if nit >= maxiter:
                task[0], task[1] = 5, 504
            elif nfev > maxfun:
                task[0], task[1] = 5, 502
        else:
            break
    msg = {4: "CONVERGENCE", 5: "STOP", 6: "WARNING", 7: "ERROR", 8: "ABNORMAL"}.get(int(task[0]), str(int(task[0])))
    return x, float(f), {"task": f"{msg} ({int(task[1])})", "nit": nit, "funcalls": nfev, "grad": g}


def _lbfgsb_box(fg, x0, m, factr, pgtol, maxiter, maxfun, callback):
    """L-BFGS-B on the box [0, 1]^n: the library's own implementation (default), or scipy's build of the reference's lbfgsb.f with
    SMASHX_LBFGSB=scipy."""
    import os
    if os.environ.get("SMASHX_LBFGSB", "native") == "scipy":
        return _lbfgsb_scipy(fg, x0, m, factr, pgtol, maxiter, maxfun, callback)
    return _lbfgsb_native(fg, x0, m, factr, pgtol, maxiter, maxfun, callback)


def wjreg_range(wjreg_opt, nb_wjreg_lcurve):
    """Regularisation weights tried by the L-curve, centred on the `fast` estimate (core/simulation/_optimize.py:911-945,
    `_compute_wjreg_range`): five weights a third of a decade apart around it, and for nb_wjreg_lcurve > 6 whole decades
    below and above (the extra cycles split half / half, the odd one above).  float32 like the reference's."""
    centre = np.log10(wjreg_opt)
    span = 0.66
    around = np.array(10 ** np.arange(centre - span, centre + span + 0.01, span / 2), dtype=np.float32)
    extra = int(nb_wjreg_lcurve) - 6
    if extra <= 0:
        return around
    below_from = centre - span - (extra - np.ceil(extra / 2.0))
    above_to = centre + span + 1.0 + (extra - np.floor(extra / 2.0))
    below = np.array(10 ** np.arange(below_from, centre - span), dtype=np.float32)
    above = np.array(10 ** np.arange(centre + span + 1.0, above_to), dtype=np.float32)
    return np.hstack((below, around, above))


def best_lcurve_weight(cost_jobs, cost_jreg, wjreg, jobs_min, jobs_max, jreg_min, jreg_max):
    """The weight at the corner of the L-curve (core/simulation/_optimize.py:948-1003, `_compute_best_lcurve_weight`).  In the
    plane x = share of the attainable misfit reduction a cycle kept, y = share of the largest regularisation term it paid, the
    corner is the point farthest below the diagonal y = x, measured the reference's way: hyp * sin(pi/4 - acos(x / hyp)) with
    hyp = sqrt(x^2 + y^2).  Operand types are the caller's (the reference's cycles hand float32 arrays and float32 extrema), so
    the `y < x` test next to the diagonal and the `>=` tie-break (of equal distances the LAST wins) fall as they do there.
    Points on or above the diagonal get NaN, cycles that did not reduce the misfit 0.  Returns (distance float32 array, weight
    or None)."""
    cost_jobs, cost_jreg = np.asarray(cost_jobs), np.asarray(cost_jreg)
    if not (cost_jobs.size > 2 and (jreg_max - jreg_min) > 0.0 and (jobs_max - jobs_min) > 0.0):
        return np.empty(0, np.float32), None
    x = (jobs_max - cost_jobs) / (jobs_max - jobs_min)         # element type of the inputs
    y = (cost_jreg - jreg_min) / (jreg_max - jreg_min)
    dist = np.zeros(cost_jobs.size, np.float32)
    best, far = None, 0.0
    for i in range(cost_jobs.size):
        if not (y[i] < x[i]):
            dist[i] = np.nan
            continue
        if cost_jobs[i] < jobs_max:
            hyp = (x[i] ** 2.0 + y[i] ** 2.0) ** 0.5
            dist[i] = hyp * np.sin(np.pi * 0.25 - np.arccos(x[i] / hyp))
        if dist[i] >= far:
            far, best = dist[i], wjreg[i]
    return dist, best


def auto_wjreg_cycles(run_cycle, restore, auto_wjreg, nb_wjreg_lcurve=6, verbose=False):
    """The calibration cycles behind auto_wjreg = 'fast' | 'lcurve' (core/simulation/_optimize.py:257-453, the part of
    `_optimize_lbfgsb` that chooses the weight of the regularisation term).
    run_cycle(wjreg) -> dict(cost, cost_jobs, cost_jreg, cost_jobs_initial): one complete optimize_lbfgsb with that weight;
    restore(): parameters / states back to the first guess.  Returns (wjreg chosen or None, lcurve dict or None): the last
    run_cycle call made here is the final calibration with the chosen weight (no weight chosen: the caller runs the model
    as it is, like the reference)."""
    def say(tag, w):
        if verbose:
            print(f"    {tag}: wJreg = {w:.6f}\n")

    say("CYCLE 1", 0.0)
    first = run_cycle(0.0)
    if auto_wjreg == "fast":
        # the misfit the unregularised calibration removed, per unit of regularisation term it ended with
        w = (first["cost_jobs_initial"] - first["cost_jobs"]) / first["cost_jreg"]
        restore()
        say("FINAL CYCLE", w)
        run_cycle(w)
        return w, None
    if auto_wjreg != "lcurve":
        raise ValueError(f"Unknown auto_wjreg '{auto_wjreg}'. Choices: ['fast', 'lcurve']")
    jobs_min, jobs_max, jreg_max = first["cost_jobs"], first["cost_jobs_initial"], first["cost_jreg"]
    if (jobs_min / jobs_max) < 0.95 and jreg_max > 0.0:
        w_fast = (jobs_max - jobs_min) / jreg_max
        tries = wjreg_range(w_fast, nb_wjreg_lcurve)
    else:
        w_fast, tries = 0.0, np.empty(0, np.float32)
    rec = {k: np.zeros(tries.size + 1, np.float32) for k in ("cost", "cost_jobs", "cost_jreg", "wjreg")}
    for k in ("cost", "cost_jobs", "cost_jreg"):
        rec[k][0] = first[k]
    for i, w in enumerate(tries):
        restore()
        say(f"CYCLE {i + 2}", w)
        r = run_cycle(w)
        for k in ("cost", "cost_jobs", "cost_jreg"):
            rec[k][i + 1] = r[k]
        rec["wjreg"][i + 1] = w
    jobs_min, jobs_max = np.min(rec["cost_jobs"]), np.max(rec["cost_jobs"])
    jreg_min, jreg_max = np.min(rec["cost_jreg"]), np.max(rec["cost_jreg"])
    dist, w_best = best_lcurve_weight(rec["cost_jobs"], rec["cost_jreg"], rec["wjreg"], jobs_min, jobs_max, jreg_min, jreg_max)
    lcurve = {"cost_jobs_initial": jobs_max, "cost_jreg_initial": jreg_min, "wjreg_lcurve_opt": w_best, "wjreg_fast": w_fast,
              "wjreg": rec["wjreg"], "distance": dist, "cost": rec["cost"], "cost_jobs": rec["cost_jobs"], "cost_jreg": rec["cost_jreg"]}
    restore()
    if w_best is not None:
        say("FINAL CYCLE", w_best)
        run_cycle(w_best)
    return w_best, lcurve


def optimize_lbfgsb(setup, mesh, input_data, parameters, states, output, verbose=False, auto_wjreg=None, nb_wjreg_lcurve=6,
                    return_lcurve=False, decomposition=None):
    """In-place like the reference: parameters / states come back calibrated (denormalised), output holds the final run.
    Returns a dict with the cost trajectory.  setup.optimize.maxiter bounds the iterations (default 100).
    auto_wjreg = 'fast' | 'lcurve' (only with jreg_fun set): the weight of the regularisation term is found by calibration
    cycles first (auto_wjreg_cycles above) and left in setup.optimize.wjreg; the returned dict is the final cycle's, with
    'wjreg' and, for return_lcurve, 'lcurve' added.

    decomposition (multi-GPU, smash_amd.tiles.Decomposition): the calibration over the ranks of a tile decomposition.  Every rank
    calls this function with ITS setup / mesh (its gauges), whole-grid parameter planes and input_data._smashx_solver = the
    plan of its part (exchange set).  The control vector is the whole grid's, in the reference's order; rank 0 runs L-BFGS-B and
    hands every trial point to the others, each evaluation is one collective forward_b: the parts' cost_jobs are summed, the
    regulariser's term -- evaluated over the whole grid by every rank -- counted once, every rank contributes the gradient of the
    cells it owns.  The iterates are those of the single domain (the sweep is bit-identical, the sums are not reordered).
    auto_wjreg works over a decomposition too: every cycle is a collective calibration and every rank takes the same decisions."""
    if auto_wjreg is not None and setup.optimize.njr > 0:
        o = setup.optimize
        if auto_wjreg == "lcurve" and nb_wjreg_lcurve < 6:
            raise ValueError("nb_wjreg_lcurve option must be greater or equal to 6")
        par0, sta0 = parameters.copy(), states.copy()
        last = {}

        def restore():
            for k in PARAM_NAMES:
                setattr(parameters, k, np.asfortranarray(getattr(par0, k)).copy(order="F"))
            for k in STATE_NAMES:
                setattr(states, k, np.asfortranarray(getattr(sta0, k)).copy(order="F"))

        def run_cycle(w):
            o.wjreg = float(w)
            # over a decomposition every cycle is a collective calibration; what the cycles decide on -- the decomposition's cost_jobs
            # (all-reduced), the common cost_jreg, the initial cost_jobs -- is the same numbers on every rank, so every rank tries the
            # same weights and picks the same one
            h = optimize_lbfgsb(setup, mesh, input_data, parameters, states, output, verbose=verbose, decomposition=decomposition)
            last["h"] = h
            return dict(cost=output.cost, cost_jobs=output.cost_jobs, cost_jreg=output.cost_jreg, cost_jobs_initial=h["cost_jobs_initial"])

        w, lcurve = auto_wjreg_cycles(run_cycle, restore, auto_wjreg, nb_wjreg_lcurve, verbose)
        if w is None:
            # no corner found: the model is run as it is; like the reference, wjreg stays at the last weight a cycle tried
            # (core/simulation/_optimize.py:434-450 does not reset it), so output.cost carries that weight's regularisation term
            forward(setup, mesh, input_data, parameters, parameters.copy(), states, states.copy(), output, np.float32(0))
            if decomposition is not None:
                v = np.array([float(output.cost_jobs)], np.float64)
                decomposition.allreduce(v)
                output.cost_jobs = np.float32(v[0])
                output.cost = np.float32(np.float32(v[0]) + np.float32(o.wjreg) * np.float32(output.cost_jreg))
        h = dict(last["h"], wjreg=w)
        if return_lcurve and lcurve is not None:
            h["lcurve"] = lcurve
        return h
    o = setup.optimize
    maxiter = int(getattr(o, "maxiter", 100))
    act = np.asarray(mesh.active_cell) == 1
    mask_f = act.reshape(-1, order="F")                    # column outer, row inner = the reference's control-vector order
    pf = [k for i, k in enumerate(PARAM_NAMES) if o.optim_parameters[i] > 0]
    sf = [k for i, k in enumerate(STATE_NAMES) if o.optim_states[i] > 0]
    m = int(np.count_nonzero(mask_f))
    n = m * (len(pf) + len(sf))
    if n == 0:
        raise ValueError("nothing to optimise: optim_parameters / optim_states are all zero")

    _normalize(parameters, PARAM_NAMES, o.lb_parameters, o.ub_parameters)
    _normalize(states, STATE_NAMES, o.lb_states, o.ub_states)
    par_bgd, sta_bgd = parameters.copy(), states.copy()
    par_b, sta_b = parameters.copy(), states.copy()
    was = o.denormalize_forward
    o.denormalize_forward = True

    def flat(obj, k):
        a = getattr(obj, k)
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.f_contiguous):
            a = np.asfortranarray(a, dtype=np.float32)
            setattr(obj, k, a)
        return a.reshape(-1, order="F")                   # a view of the Fortran-ordered field

    def to_control(p, s):
        return np.concatenate([flat(p, k)[mask_f].astype(np.float64) for k in pf] + [flat(s, k)[mask_f].astype(np.float64) for k in sf])

    def to_var(x):
        for j, k in enumerate(pf):
            flat(parameters, k)[mask_f] = x[j * m:(j + 1) * m]
        for j, k in enumerate(sf):
            flat(states, k)[mask_f] = x[(len(pf) + j) * m:(len(pf) + j + 1) * m]

    def renormalize():
        _normalize(parameters, PARAM_NAMES, o.lb_parameters, o.ub_parameters)
        _normalize(states, STATE_NAMES, o.lb_states, o.ub_states)

    hist = {"cost": [], "nfg": 0}
    x = to_control(parameters, states)
    moved = set(pf + sf)
    dec = decomposition
    if dec is not None:
        own_f = np.asarray(dec.owned, bool).reshape(-1, order="F")[mask_f]          # control-vector order
        own_ctl = np.tile(own_f, len(pf) + len(sf))

    def whole_cost():
        """the decomposition's cost from this rank's output: sum of the parts' cost_jobs + wjreg x the (common) cost_jreg"""
        if dec is None:
            return float(np.float32(output.cost))
        v = np.array([float(output.cost_jobs)], np.float64)
        dec.allreduce(v)
        output.cost_jobs = np.float32(v[0])
        output.cost = np.float32(np.float32(v[0]) + np.float32(o.wjreg) * np.float32(output.cost_jreg))
        return float(output.cost)

    try:
        forward(setup, mesh, input_data, parameters, par_bgd, states, sta_bgd, output, np.float32(0))
        renormalize()
        whole_cost()
        hist["cost_jobs_initial"], hist["cost_jreg_initial"] = output.cost_jobs, output.cost_jreg
        last = {}
        # every evaluation is one forward_b with denormalize_forward on (mw_optimize.f90:590-606).  The plan keeps the fields
        # that do not move on the device: an evaluation uploads the optimised fields only and brings back cost, discharge
        # and the gradient of those fields -- nothing is denormalised and renormalised on the host in between.
        sol = _solver_for(setup, mesh, input_data)
        sol.upload(parameters, states, par_bgd, sta_bgd)

        device_pack = dec is None and sol.control_size() == n       # control_to_var / var_to_control on the device (smashx_control_*)

        def fg(xc):
            if dec is not None:
                # one collective evaluation: rank 0's trial point on every rank, the parts' costs and gradients put together
                xc = dec.bcast_point(xc)
                to_var(xc)
                sol.upload(parameters, states, par_bgd, sta_bgd, only=moved)
                sol.sweep(True, 1.0)
                sol.download(True, None, None, output, par_b, sta_b, only_b=moved)
                g = to_control(par_b, sta_b)
                g[~own_ctl] = 0.0                                   # (cells of other parts carry the regulariser's gradient here too)
                dec.allreduce(g)
                hist["nfg"] += 1
                last["f"], last["g"] = whole_cost(), g
                return last["f"], g
            if device_pack:
                # mw_optimize.f90:590-606 with the packing on the device: one contiguous fp64 vector goes up, the fields are
                # unpacked, cast and denormalised there; cost + discharge and one contiguous gradient vector come back
                sol.control_set(xc)
                sol.sweep(True, 1.0)
                sol.cost_and_qsim(output)
                g = sol.control_gradient()
            else:
                to_var(xc)
                sol.upload(parameters, states, par_bgd, sta_bgd, only=moved)
                sol.sweep(True, 1.0)
                sol.download(True, None, None, output, par_b, sta_b, only_b=moved)
                g = to_control(par_b, sta_b)
            hist["nfg"] += 1
            last["f"], last["g"] = float(np.float32(output.cost)), g
            return last["f"], g

        def cb(xk, pg=None):
            hist["cost"].append(last["f"])
            if verbose:
                print(f"    At iterate {len(hist['cost']):3d}    nfg = {hist['nfg']:5d}    J = {last['f']:14.6f}")
            if pg is None:
                pg = np.max(np.abs(xk - np.clip(xk - last["g"], 0.0, 1.0)))   # |proj g| (lbfgsb.f projgr)
            if pg <= 1e-10 * (1.0 + abs(last["f"])):
                last["x"] = xk.copy()
                raise _Stop

        cb.wants_pg = True
        if dec is None or dec.rank == 0:
            try:
                x, f, info = _lbfgsb_box(fg, x, 10, 10.0, 1e-12, maxiter, 10 * maxiter + 20, cb)
                hist["task"] = str(info.get("task", ""))
            except _Stop:
                x = last["x"]
                hist["task"] = "STOP: THE PROJECTED GRADIENT IS SUFFICIENTLY SMALL"
            if dec is not None:
                x = dec.bcast_point(x, done=True)
        else:
            # the other ranks evaluate what rank 0 asks for until it says the search is over
            while True:
                xw = dec.bcast_point(None)
                if xw is None:
                    break
                fg(_Held(xw))
            x = dec.final_point
        to_var(x)
        forward(setup, mesh, input_data, parameters, par_bgd, states, sta_bgd, output, np.float32(0))
        hist["final_cost"] = whole_cost()
    finally:
        o.denormalize_forward = was
    return hist


# ---- uniform calibration: mw_optimize::optimize_sbs (mw_optimize.f90:53-294) -----------------------------------------------------------
# "auto" takes the catchment-resident kernel for a batch of at least this many candidates, when smashx_uniform_costs accepts the plan
# and the options.  Measured (profiles/uniform_costs.json): a resident call costs one launch whatever the batch -- 2.6 ms
# on Cance, 17.5 ms on 32 x 32 x 8760 -- and a forward of the loop 1.45 ms / 8.5 ms, so the loop wins for 1 candidate (the line-search
# point of an iteration), 2 are a tie (Cance to the kernel, the synthetic case to the loop, both by less than 10 %) and the kernel wins from 3.
SBS_AUTO_MIN_CANDIDATES = 3


def optimize_sbs(setup, mesh, input_data, parameters, states, output, verbose=False, candidates="auto"):
    """The mirror of mw_optimize::optimize_sbs, the reference's default calibration (mapping="uniform", algorithm="sbs"): in place,
    parameters / states come back with the calibrated value of every optimised field on the active cells (inactive cells keep
    theirs), output holds the final run.  The control vector and its bounds are the fields flagged in setup.optimize.optim_parameters
    / optim_states with lb_* / ub_* in stacked order (bounds_initialise_sbs), the start point is read at the first active cell in
    column-major order (var_to_control_sbs), setup.optimize.maxiter bounds the iterations (default 100).  The optimiser is the
    library's (smashx_sbs_*: the reference's loop restated in fp32, ask / tell); the initial and the final evaluation are forward().

    candidates: how the batch of candidates of a stage is evaluated -- "resident": smashx_uniform_costs, one workgroup per candidate;
    "ensemble": smashx_multiple_run; "loop": one forward per candidate; "auto": resident when it accepts the plan and the options and
    the batch has SBS_AUTO_MIN_CANDIDATES candidates, else the loop.  The three give the same costs bit for bit, hence the same
    trajectory.  Returns a dict: per completed iterate k (the reference's iter / n) the cost, the point, nfg and ddx; the message."""
    import ctypes as C
    from . import _lib
    from .solver import FIELD_NAMES
    if candidates not in ("auto", "resident", "ensemble", "loop"):
        raise ValueError(f"candidates must be 'auto', 'resident', 'ensemble' or 'loop', not {candidates!r}")
    o = setup.optimize
    maxiter = int(getattr(o, "maxiter", 100))
    optim = list(np.asarray(o.optim_parameters).reshape(-1)) + list(np.asarray(o.optim_states).reshape(-1))
    lb = list(np.asarray(o.lb_parameters, np.float32).reshape(-1)) + list(np.asarray(o.lb_states, np.float32).reshape(-1))
    ub = list(np.asarray(o.ub_parameters, np.float32).reshape(-1)) + list(np.asarray(o.ub_states, np.float32).reshape(-1))
    fields = [i for i in range(len(FIELD_NAMES)) if optim[i] > 0]
    n = len(fields)
    if n == 0:
        raise ValueError("nothing to optimise: optim_parameters / optim_states are all zero")
    names = [FIELD_NAMES[i] for i in fields]
    ind = np.array([i + 1 for i in fields], np.int32)
    lower = np.array([lb[i] for i in fields], np.float32)
    upper = np.array([ub[i] for i in fields], np.float32)
    act = np.asarray(mesh.active_cell) == 1
    if not act.any():
        raise ValueError("the mesh has no active cell")
    first = int(np.argmax(act.reshape(-1, order="F")))         # maxloc(mesh%active_cell): the first active cell, column-major
    r0, c0 = first % act.shape[0], first // act.shape[0]

    def holder(k):
        return parameters if k in PARAM_NAMES else states

    def plane(obj, k):
        a = getattr(obj, k)
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.f_contiguous):
            a = np.asfortranarray(a, dtype=np.float32)
            setattr(obj, k, a)
        return a

    def control_to_var(par, sta, x):           # where (mask) matrix(:, :, i) = x(j)
        for k, v in zip(names, x):
            plane(par if k in PARAM_NAMES else sta, k)[act] = np.float32(v)

    x0 = np.array([plane(holder(k), k)[r0, c0] for k in names], np.float32)
    par_bgd, sta_bgd = parameters.copy(), states.copy()
    forward(setup, mesh, input_data, parameters, par_bgd, states, sta_bgd, output, np.float32(0))
    cost0 = np.float32(output.cost)
    hist = {"cost": [float(cost0)], "x": [x0.copy()], "nfg": [1], "ddx": [0.64], "fields": names, "task": "", "route": candidates}
    if verbose:
        print(f"    At iterate    {0:3d}    nfg = {1:5d}    J ={float(cost0):10.6f}    ddx ={0.64:5.2f}")

    sol = _solver_for(setup, mesh, input_data)
    route = {"use": candidates}
    trial_par, trial_sta = parameters.copy(), states.copy()

    def costs_of(y):
        m = y.shape[1]
        use = route["use"]
        if use == "auto":
            use = "resident" if m >= SBS_AUTO_MIN_CANDIDATES else "loop"
        if use == "resident":
            try:
                return sol.uniform_costs(parameters, states, y, ind)
            except _lib.SmashxError as e:
                if route["use"] != "auto" or e.code != _lib.E_UNSUPPORTED:
                    raise
                route["use"] = "loop"           # signature criteria, a regulariser, a catchment over the kernel's limits: the loop runs them all
                hist["route"] = "auto -> loop: " + str(e)
        elif use == "ensemble":
            return sol.multiple_run(parameters, states, y, ind)
        f = np.zeros(m, np.float32)
        for c in range(m):
            control_to_var(trial_par, trial_sta, y[:, c])
            forward(setup, mesh, input_data, trial_par, par_bgd, trial_sta, sta_bgd, output, np.float32(0))
            f[c] = np.float32(output.cost)
        return f

    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.smashx_sbs_create(n, lower.ctypes.data, upper.ctypes.data, x0.ctypes.data, C.c_float(float(cost0)), maxiter, C.byref(h)))
    try:
        ybuf = np.zeros((n, 2 * n), np.float32, order="F")
        m = C.c_int(0)
        x = x0.copy()
        done = 0
        while True:
            _lib.check(L.smashx_sbs_ask(h, ybuf.ctypes.data, C.byref(m)))
            if m.value == 0:
                break
            f = np.ascontiguousarray(costs_of(np.asfortranarray(ybuf[:, :m.value])), np.float32)
            _lib.check(L.smashx_sbs_tell(h, f.ctypes.data))
            it = L.smashx_sbs_iter(h)
            if it != done:
                done = it
                _lib.check(L.smashx_sbs_x(h, x.ctypes.data))
                control_to_var(parameters, states, x)           # the base of the next stage's candidates is the current point
                control_to_var(trial_par, trial_sta, x)
                if it % n == 0:
                    gx, ddx, nfg = float(L.smashx_sbs_gx(h)), float(L.smashx_sbs_ddx(h)), int(L.smashx_sbs_nfg(h))
                    hist["cost"].append(gx); hist["x"].append(x.copy()); hist["nfg"].append(nfg); hist["ddx"].append(ddx)
                    if verbose:
                        print(f"    At iterate    {it // n:3d}    nfg = {nfg:5d}    J ={gx:10.6f}    ddx ={ddx:5.2f}")
        hist["task"] = L.smashx_sbs_message(h).decode()
        hist["iter"], hist["nfg_total"] = int(L.smashx_sbs_iter(h)), int(L.smashx_sbs_nfg(h))
        if hist["task"]:           # one of the reference's two stopping rules: the final evaluation at x
            if verbose:
                print("    " + hist["task"] + "\n")
            _lib.check(L.smashx_sbs_x(h, x.ctypes.data))
            control_to_var(parameters, states, x)
            forward(setup, mesh, input_data, parameters, par_bgd, states, sta_bgd, output, np.float32(0))
        hist["final_cost"], hist["final_x"] = float(np.float32(output.cost)), x.copy()
    finally:
        L.smashx_sbs_destroy(h)
    return hist


# ---- regionalisation: mw_optimize::optimize_hyper_lbfgsb (mw_optimize.f90:779-1177) ---------------------------------------------------
def _logf(x):
    """logf of the C library, which the reference's compiled code calls (numpy's float32 log is another implementation)"""
    import ctypes as C
    import ctypes.util
    lm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lm.logf.restype, lm.logf.argtypes = C.c_float, [C.c_float]
    return np.float32(lm.logf(C.c_float(float(x))))


def hyper_problem_initialise(setup, mesh, parameters, states):
    """problem_initialise_hyper_lbfgsb + var_to_control_hyper_lbfgsb (mw_optimize.f90:1001-1135).  Returns (hyper_parameters,
    hyper_states, x0, l, u, nbd): the first row of every column is the inverse sigmoid of the field at maxloc(active_cell) (fp32,
    both operands floored at 1e-8), every other coefficient 0; the exponents of a flagged field under hyper-polynomial start at 1 with
    bounds [0.5, 2] (nbd = 2), everything else is unbounded (nbd = 0, l = u = 0 as the reference leaves them).  The control is the
    flagged columns, parameters before states."""
    from .types import Hyper_ParametersDT, Hyper_StatesDT
    o = setup.optimize
    nh = int(o.nhyper)
    flat = int(np.argmax(np.asarray(mesh.active_cell).reshape(-1, order="F")))        # maxloc: the first maximum in array element order
    r, c = flat % mesh.nrow, flat // mesh.nrow
    f32 = np.float32
    H = np.zeros((nh, len(PARAM_NAMES) + len(STATE_NAMES)), f32, order="F")
    vals = [getattr(parameters, k)[r, c] for k in PARAM_NAMES] + [getattr(states, k)[r, c] for k in STATE_NAMES]
    lb = np.concatenate([np.asarray(o.lb_parameters, f32), np.asarray(o.lb_states, f32)])
    ub = np.concatenate([np.asarray(o.ub_parameters, f32), np.asarray(o.ub_states, f32)])
    for i, v in enumerate(vals):
        v = f32(v)
        H[0, i] = _logf(max(f32(1e-8), f32(v - lb[i])) / max(f32(1e-8), f32(ub[i] - v)))
    optim = np.concatenate([np.asarray(o.optim_parameters), np.asarray(o.optim_states)]) > 0
    n = int(np.count_nonzero(optim)) * nh
    l, u, nbd = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    k = 0
    for i in np.flatnonzero(optim):
        if o.mapping == "hyper-polynomial":
            for j in range(2, nh, 2):                       # rows 3, 5, ... of the column (1-based): the exponents
                H[j, i] = 1.0
                nbd[k + j], l[k + j], u[k + j] = 2, 0.5, 2.0
        k += nh
    HP, HS = Hyper_ParametersDT(setup), Hyper_StatesDT(setup)
    HP.set_matrix(H[:, :len(PARAM_NAMES)])
    HS.set_matrix(H[:, len(PARAM_NAMES):])
    x0 = np.concatenate([H[:, i].astype(np.float64) for i in np.flatnonzero(optim)]) if n else np.zeros(0, np.float64)
    return HP, HS, x0, l, u, nbd


def optimize_hyper_lbfgsb(setup, mesh, input_data, parameters, states, output, verbose=False, device_map=True, evaluate=None):
    """Mirror of mw_optimize::optimize_hyper_lbfgsb (mw_optimize.f90:779-958): the coefficients of the descriptor -> field maps
    (setup.optimize.mapping = "hyper-linear" | "hyper-polynomial", nhyper rows per field) calibrated by L-BFGS-B with m = 10,
    factr = 1e6, pgtol = 1e-12, the bounds of hyper_problem_initialise, stopped at setup.optimize.maxiter iterations or when
    |proj g| <= 1e-10 (1 + |f|).  ALL 24 fields are mapped; the flagged ones form the control, parameters before states.  The
    descriptors are normalised by their whole-grid minimum and maximum for the calibration and put back afterwards (exactly as they
    were; the reference recomputes them from the normalised values).  In place like the reference: parameters / states come back as
    the mapped fields of the calibrated coefficients over the WHOLE grid, output holds the final hyper_forward run.

    device_map = True: every evaluation is hyper_upload -> adjoint sweep -> hyper_gradient on the device (include/smashx_hyper.h) --
    two small matrices go up, two come back; False: the host composition smash_amd.hyper_forward_b (planes over PCIe, the maps of
    sx_hyper.cpp), which computes the same numbers bit for bit.  evaluate(hyper_parameters, hyper_states) -> (cost, hyper_parameters_b
    matrix, hyper_states_b matrix) replaces both, and the final run with them (the loop can then be driven without a GPU; the
    descriptors it sees in input_data are the normalised ones).

    Returns the history dict of optimize_lbfgsb (cost per iterate, nfg, task, final_cost) plus cost_initial, x0 / l / u / nbd and
    the final matrices hyper_parameters (nhyper, 16) / hyper_states (nhyper, 8)."""
    from .solver import _hyper_to_fields, _plain, hyper_forward, hyper_forward_b
    o = setup.optimize
    if o.mapping not in ("hyper-linear", "hyper-polynomial"):
        raise ValueError(f"setup.optimize.mapping = {o.mapping!r}: hyper-linear or hyper-polynomial expected")
    maxiter = int(getattr(o, "maxiter", 100))
    optim = np.concatenate([np.asarray(o.optim_parameters), np.asarray(o.optim_states)]) > 0
    if not optim.any():
        raise ValueError("nothing to optimise: optim_parameters / optim_states are all zero")
    nh, npar = int(o.nhyper), len(PARAM_NAMES)

    # normalize_descriptor_hyper_lbfgsb (:960-980), fp32
    desc0 = input_data.descriptor
    desc = np.asfortranarray(desc0, dtype=np.float32).copy(order="F")
    for i in range(desc.shape[2]):
        lo, hi = desc[:, :, i].min(), desc[:, :, i].max()
        desc[:, :, i] = (desc[:, :, i] - lo) / (hi - lo)
    input_data.descriptor = desc
    try:
        HP, HS, x0, l, u, nbd = hyper_problem_initialise(setup, mesh, parameters, states)
        hist = {"cost": [], "nfg": 0, "x0": x0.copy(), "l": l, "u": u, "nbd": nbd}
        last = {}
        injected = evaluate is not None
        if not injected and device_map:
            sol = _solver_for(_plain(setup), mesh, input_data)
            sol.set_hyper_descriptors(o.mapping, desc)

            def evaluate(hp, hs):
                sol.hyper_upload(hp, hs)
                sol.sweep(True, 1.0)
                cost = sol.cost_and_qsim(output)
                hpb, hsb = sol.hyper_gradient()
                return cost, hpb, hsb
        elif not injected:
            par_b, sta_b = parameters.copy(), states.copy()

            def evaluate(hp, hs):
                HPb, HSb = HP.copy(), HS.copy()
                cost = hyper_forward_b(setup, mesh, input_data, parameters, par_b, HP, HPb, HP, states, sta_b, HS, HSb, HS, output, None,
                                       np.float32(0), np.float32(1))
                return cost, HPb.matrix(), HSb.matrix()

        def to_var(x):
            # control_to_var_hyper_lbfgsb (:1137-1177): real(x(k), sp) into the flagged columns
            M = np.concatenate([HP.matrix(), HS.matrix()], axis=1)
            for j, i in enumerate(np.flatnonzero(optim)):
                M[:, i] = np.asarray(x[j * nh:(j + 1) * nh], np.float64).astype(np.float32)
            HP.set_matrix(M[:, :npar])
            HS.set_matrix(M[:, npar:])

        def fg(x):
            to_var(x)
            cost, hpb, hsb = evaluate(HP.matrix(), HS.matrix())
            G = np.concatenate([np.asarray(hpb, np.float32), np.asarray(hsb, np.float32)], axis=1)
            g = np.concatenate([G[:, i].astype(np.float64) for i in np.flatnonzero(optim)])
            hist["nfg"] += 1
            last["f"], last["g"] = float(np.float32(cost)), g
            if hist["nfg"] == 1:
                hist["cost_initial"] = last["f"]
            return last["f"], g

        def cb(xk, pg=None):
            hist["cost"].append(last["f"])
            if verbose:
                print(f"    At iterate {len(hist['cost']):3d}    nfg = {hist['nfg']:5d}    J = {last['f']:14.6f}")
            if pg is not None and pg <= 1e-10 * (1.0 + abs(last["f"])):
                last["x"] = xk.copy()
                raise _Stop

        cb.wants_pg = True
        lower = np.where(nbd == 2, l, -np.inf)
        upper = np.where(nbd == 2, u, np.inf)
        try:
            x, f, info = _lbfgsb_native(fg, x0, 10, 1e6, 1e-12, maxiter, 1 << 30, cb, lower, upper)
            hist["task"] = str(info.get("task", ""))
        except _Stop:
            x = last["x"]
            hist["task"] = "STOP: THE PROJECTED GRADIENT IS SUFFICIENTLY SMALL"
        to_var(x)
        # the final hyper_forward (:950-954); the caller's planes are then mapped over the whole grid, inactive cells included, as
        # hyper_parameters_to_parameters / hyper_states_to_states leave them
        if injected:
            hist["final_cost"] = float(np.float32(evaluate(HP.matrix(), HS.matrix())[0]))
        elif device_map:
            sol.hyper_upload(HP.matrix(), HS.matrix())
            sol.sweep(False)
            hist["final_cost"] = float(np.float32(sol.download(False, None, None, output)))
        else:
            hist["final_cost"] = float(np.float32(hyper_forward(setup, mesh, input_data, parameters, HP, HP, states, HS, HS, output,
                                                                np.float32(0))))
        _hyper_to_fields(setup, mesh, input_data, parameters, HP, states, HS)
        hist["hyper_parameters"], hist["hyper_states"] = HP.matrix(), HS.matrix()
    finally:
        input_data.descriptor = desc0
    return hist


# ---- regionalisation by a neural network: Model.ann_optimize (smash/core/simulation/_ann_optimize.py, net.py:353-415) ------------------
def ann_auto_graph(ntrain, nd, control_vector, bounds, optimizer="adam", learning_rate=0.003, random_state=None):
    """_set_graph's network for net = None (_ann_optimize.py:140-175): dense(round(sqrt(ntrain nd) 2/3)) relu, dense(half of it) relu,
    dense(ncv) sigmoid, scale(bounds), glorot_uniform kernels, compiled with the optimizer"""
    from .net import Net
    net = Net()
    n_neurons = round(np.sqrt(ntrain * nd) * 2 / 3)
    net.add(layer="dense", options={"input_shape": (nd,), "neurons": n_neurons, "kernel_initializer": "glorot_uniform"})
    net.add(layer="activation", options={"name": "relu"})
    net.add(layer="dense", options={"neurons": round(n_neurons / 2), "kernel_initializer": "glorot_uniform"})
    net.add(layer="activation", options={"name": "relu"})
    net.add(layer="dense", options={"neurons": len(control_vector), "kernel_initializer": "glorot_uniform"})
    net.add(layer="activation", options={"name": "sigmoid"})
    net.add(layer="scale", options={"bounds": bounds})
    net.compile(optimizer=optimizer, random_state=random_state, options={"learning_rate": learning_rate})
    return net


def ann_optimize(setup, mesh, input_data, parameters, states, output, control_vector, bounds, net=None, optimizer="adam",
                 learning_rate=0.003, epochs=400, early_stopping=False, random_state=None, verbose=False, device_map=True, evaluate=None):
    """Mirror of _ann_optimize + Net._fit_d2p: a network maps the descriptors of a cell to the control fields (control_vector: names of
    parameters / states, bounds (ncv, 2)); its weights are trained for `epochs` epochs on the cost of one adjoint run per epoch, by the
    net's optimizer.  The descriptors are normalised in fp32 by their whole-grid minimum and maximum for the training and handed back
    exactly as they were.  net = None builds the reference's graph (ann_auto_graph).  early_stopping keeps the weights of the epoch
    with the lowest cost.  In place like the reference: the control fields come back as the network's outputs -- of the last epoch's
    forward pass at the active cells, of the final weights elsewhere --, output holds the last epoch's run, net.history["loss_train"]
    the cost per epoch.  Returns the net.

    device_map = True: an epoch is ann_upload -> adjoint sweep -> ann_gradient on the device (include/smashx_ann.h); only the weights and
    their gradient cross PCIe.  False: the host composition -- the host network (smashx_ann_host_*), forward_b, planes over PCIe --,
    which computes the same bits.  A regulariser (setup.optimize.jreg_fun) is refused on the device path (SMASHX_E_UNSUPPORTED); the
    host composition runs it against the fields as they were before the training, like the reference.  evaluate(planes) -> (cost, gradient planes), both dicts name -> (nrow, ncol) plane over the control
    vector, replaces the sweep of the host composition (the loop can then run without a GPU).

    The rows of the training set and the weight-gradient sums follow the active cells in column-major order (csrc/sx_ann.h); the
    reference takes them in row-major order, which is the same mathematics in another order of summation."""
    from .net import Net
    from .solver import forward_b
    control_vector = [str(k) for k in control_vector]
    bounds = np.asarray(bounds, np.float64).reshape(len(control_vector), 2)
    o = setup.optimize
    for name, (lo, hi) in zip(control_vector, bounds):          # _ann_optimize.py:43-59
        if name in PARAM_NAMES:
            i = PARAM_NAMES.index(name)
            o.optim_parameters[i], o.lb_parameters[i], o.ub_parameters[i] = 1, lo, hi
        elif name in STATE_NAMES:
            i = STATE_NAMES.index(name)
            o.optim_states[i], o.lb_states[i], o.ub_states[i] = 1, lo, hi
        else:
            raise ValueError(f"control vector: {name!r} is neither a parameter nor a state")

    desc0 = input_data.descriptor
    desc = np.asfortranarray(desc0, dtype=np.float32).copy(order="F")
    nd = desc.shape[2]
    for i in range(nd):                                         # _normalize_descriptor (_optimize.py:801-810), fp32
        lo, hi = np.amin(desc[..., i]), np.amax(desc[..., i])
        desc[..., i] = (desc[..., i] - lo) / (hi - lo)
    active = np.asarray(mesh.active_cell) == 1
    cc, rr = np.nonzero(active.T)                               # the active cells in column-major order
    ci, ri = np.nonzero(~active.T)
    x_train, x_inactive = np.ascontiguousarray(desc[rr, cc]), np.ascontiguousarray(desc[ri, ci])

    if net is None:
        net = ann_auto_graph(len(x_train), nd, control_vector, bounds, optimizer, learning_rate, random_state)
    elif not isinstance(net, Net):
        raise ValueError(f"Unknown network {net}")
    elif not net.layers:
        raise ValueError("The graph has not been set yet")
    else:
        ips, ios = net.layers[0].input_shape, net.layers[-1].output_shape()
        if ips[0] != nd:
            raise ValueError(f"Inconsistent value between the number of input layer ({ips}) and the number of descriptors ({nd}): {ips[0]} != {nd}")
        if ios[0] != len(control_vector):
            raise ValueError(f"Inconsistent value between the number of output layer ({ios}) and the number of control vectors "
                             f"({len(control_vector)}): {ios[0]} != {len(control_vector)}")
    if not net._compiled:
        raise ValueError("The network has not been compiled yet")

    def plane_of(name):
        return getattr(parameters if name in PARAM_NAMES else states, name)

    def set_planes(y, r, c):
        for i, name in enumerate(control_vector):
            plane_of(name)[r, c] = y[:, i]

    injected = evaluate is not None
    input_data.descriptor = desc
    try:
        if not injected and device_map:
            sol = _solver_for(setup, mesh, input_data)
            sol.set_ann_descriptors(desc)
            sol.set_ann_net(net, control_vector)
            sol.upload(parameters, states, parameters, states)
        elif not injected:
            par_b, sta_b = parameters.copy(), states.copy()
            par_bgd, sta_bgd = parameters.copy(), states.copy()        # the background of every epoch: the fields before the training
        loss_opt, best = 0, None
        for epo in range(int(epochs)):
            w = net.weights()
            if not injected and device_map:
                sol.ann_upload(w)
                sol.sweep(True, 1.0)
                loss = sol.cost_and_qsim(output)
                grad = sol.ann_gradient()
            else:
                set_planes(net._forward_pass(x_train), rr, cc)
                if injected:
                    loss, gp = evaluate({k: plane_of(k) for k in control_vector})
                else:
                    loss = forward_b(setup, mesh, input_data, parameters, par_b, par_bgd, par_b, states, sta_b, sta_bgd, sta_b,
                                     output, None, np.float32(0), np.float32(1))
                    gp = {k: getattr(par_b if k in PARAM_NAMES else sta_b, k) for k in control_vector}
                loss_grad = np.stack([np.asarray(gp[k], np.float32)[rr, cc] for k in control_vector], axis=1)
                grad = net.gradient(x_train, loss_grad)
            loss = float(np.float32(loss))
            if early_stopping and (loss_opt > loss or epo == 0):
                loss_opt, best = loss, w
            net.update(grad)
            if verbose:
                print(f"    At epoch {epo + 1:3d}    J = {loss:10.6f}    |proj g| = {float(np.max(np.abs(grad))) if grad.size else 0.0:10.6f}")
            net.history["loss_train"].append(loss)
        if early_stopping and best is not None:
            net.set_weights(best)
        if not injected and device_map and int(epochs) > 0:
            sol.ann_fields(parameters, states)
        if len(x_inactive):
            set_planes(net._predict(x_inactive), ri, ci)        # the predicted map at the inactive cells, so that the planes come back whole
    finally:
        input_data.descriptor = desc0
    return net
