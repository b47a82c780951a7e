"""Records tests/golden/sbs/*.npz: the uniform step-by-step calibration of the compiled reference (mw_optimize::optimize_sbs through
oracle/refbind.run(..., optimize_sbs_maxiter=k), mode 7 of oracle/ref/ref_capi.f90) after k = 0 .. K iterations: the cost and the
calibrated values.

The reference says nothing about what happened inside a run, so the recorder restates the loop in numpy float32 with the C library's
float functions (sbs_restated below: a second statement of mw_optimize.f90:53-294, independent of smash_amd/csrc/sx_sbs.cpp), feeds
it with the costs of the plain-C oracle (bit-identical to the reference) and REFUSES a fixture unless
  * the restatement reproduces the reference's cost and values after every k bit for bit -- so its trace is the reference's -- and
  * the trace of the full fixtures holds a skipped candidate of each of the three kinds, a clipped candidate, a halving and a doubling
    of ddx, an accepted and a rejected line-search step.
nfg (which the reference only prints, and ref_capi.f90 runs it silently) is recorded from the restatement.

A full fixture also serves the default build on the GPU, whose costs differ from the reference's in their last bits and which is held to
bars (first cost 3e-7 + 1e-5 |ref|, later costs 2 %, values 2 % + 1e-3).  The optimiser's `f < gx` is a discontinuous function of the
costs, so a run that ends on a flat valley can be followed by nobody -- not by the reference itself: the first pair of full fixtures
recorded here was left by the reference's OWN build at its own optimisation level by 2.6 times those bars.  A fixture is therefore
also refused unless it is conditioned well enough by the reference's own error:
  * the reference's other build (oracle/_ref/libsmash_ref_fast.so: its own optimisation level, refbind.run(fast=True)) follows the
    recorded trajectory within the bars after every k, and
  * so does the restatement with every cost perturbed by up to the reference's flag-to-flag noise on the cost of the case (noise_cost
    of the golden file, relative), in each of NOISE_SEEDS seeded repetitions.
K is the smallest number of iterations at which the trace holds every event.

    python tests/golden/make_sbs.py            # needs oracle/_ref (built from the reference by __graft_entry__.build())
"""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "sbs")
f32 = np.float32

# name -> case, fields of the control vector, their bounds, the uniform start point, K; "needs": the events the trace must hold.
# The three transformations: exc (lower bound < 0: asinh), hp in [0, 1] (logit), cp / lr (log).
ALL = ("skip_back", "skip_lower", "skip_upper", "clipped", "halved", "doubled", "line_accepted", "line_rejected")
FIXTURES = {
    "gr_b_16x16x96_nse_gaps": dict(case="gr_b_16x16x96_nse_gaps", fields=("cp", "exc", "hp"), lb=(201.2784, -10.6121, 0.003),
                                   ub=(842.0047, 1.1225, 0.41), x0=(213.3758, -5.8927, 0.1705), K=5, needs=ALL, stop="STOP"),
    "gr_a_12x12x48_nse": dict(case="gr_a_12x12x48_nse", fields=("cp", "exc", "hp"), lb=(16.0947, -4.2266, 0.0011), ub=(520.3945, -2.2996, 0.9497),
                              x0=(453.2306, -2.901, 0.1395), K=5, needs=ALL, stop="STOP"),
    # two short ones: a run that ends by DDX < 0.01 and one that ends by maxiter
    "gr_a_12x12x48_nse_ddx": dict(case="gr_a_12x12x48_nse", fields=("lr",), lb=(1.0,), ub=(200.0,), x0=(14.0,), K=12, needs=("halved",),
                                  stop="CONVERGENCE"),
    "gr_b_16x16x96_nse_gaps_maxiter": dict(case="gr_b_16x16x96_nse_gaps", fields=("cp", "lr"), lb=(1e-6, 1e-6), ub=(1e3, 1e3), x0=(200.0, 5.0),
                                           K=2, needs=(), stop="STOP"),
}


def _libm():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for k in ("logf", "expf", "asinhf", "sinhf"):
        getattr(m, k).restype, getattr(m, k).argtypes = C.c_float, [C.c_float]
    m.powf.restype, m.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return m


def sbs_restated(cost_of, x0, l, u, maxiter, cost0):
    """mw_optimize.f90:53-294 in float32, statement by statement.  cost_of(y) -> float32.  Returns per k = iter / n the (cost, x, nfg,
    ddx), the stop message and the set of events met."""
    m = _libm()
    n = len(x0)
    log, exp, asinh, sinh = (lambda v: f32(m.logf(float(v)))), (lambda v: f32(m.expf(float(v)))), (lambda v: f32(m.asinhf(float(v)))), (lambda v: f32(m.sinhf(float(v))))
    one, zero = f32(1), f32(0)

    def tr(x):
        out = np.zeros(n, f32)
        for i in range(n):
            if l[i] < zero:
                out[i] = asinh(x[i])
            elif l[i] >= zero and u[i] <= one:
                out[i] = log(f32(x[i] / f32(one - x[i])))
            else:
                out[i] = log(x[i])
        return out

    def inv(xt):
        out = np.zeros(n, f32)
        for i in range(n):
            if l[i] < zero:
                out[i] = sinh(xt[i])
            elif l[i] >= zero and u[i] <= one:
                out[i] = f32(exp(xt[i]) / f32(one + exp(xt[i])))
            else:
                out[i] = exp(xt[i])
        return out

    x, l, u = np.array(x0, f32), np.array(l, f32), np.array(u, f32)
    x_t, l_t, u_t = tr(x), tr(l), tr(u)
    gx = f32(cost0)
    ga = gx
    clg = f32(m.powf(0.7, float(f32(one / f32(n)))))
    z_t, sdx = x_t.copy(), np.zeros(n, f32)
    ddx = f32(0.64)
    dxn = ddx
    ia = iaa = iam = jfaa = jfa = 0
    nfg = 1
    events = set()
    rows = [(gx, x.copy(), nfg, ddx)]
    msg = ""
    for it in range(1, maxiter * n + 1):
        if dxn > ddx:
            dxn = ddx
        if ddx > f32(2):
            ddx = dxn
        for i in range(1, n + 1):
            y_t = x_t.copy()
            for j in (1, 2):
                jf = 2 * j - 3
                if i == iaa and jf == -jfaa:
                    events.add("skip_back"); continue
                if x_t[i - 1] <= l_t[i - 1] and jf < 0:
                    events.add("skip_lower"); continue
                if x_t[i - 1] >= u_t[i - 1] and jf > 0:
                    events.add("skip_upper"); continue
                y_t[i - 1] = f32(x_t[i - 1] + f32(f32(jf) * ddx))
                if y_t[i - 1] < l_t[i - 1]:
                    y_t[i - 1] = l_t[i - 1]; events.add("clipped")
                if y_t[i - 1] > u_t[i - 1]:
                    y_t[i - 1] = u_t[i - 1]; events.add("clipped")
                f = f32(cost_of(inv(y_t)))
                nfg += 1
                if f < gx:
                    z_t, gx, ia, jfa = y_t.copy(), f, i, jf
        iaa, jfaa = ia, jfa
        if ia != 0:
            x_t = z_t.copy()
            x = inv(x_t)
            sdx = (clg * sdx).astype(f32)
            sdx[ia - 1] = f32(f32(f32(f32(one - clg) * f32(jfa)) * ddx) + f32(clg * sdx[ia - 1]))
            iam += 1
            if iam > 2 * n:
                ddx = f32(ddx * f32(2)); iam = 0; events.add("doubled")
            if gx < f32(ga - f32(2)):
                ga = gx
        else:
            ddx = f32(ddx / f32(2)); iam = 0; events.add("halved")
        if it > 4 * n:
            y_t = np.zeros(n, f32)
            for i in range(n):
                y_t[i] = f32(x_t[i] + sdx[i])
                if y_t[i] < l_t[i]:
                    y_t[i] = l_t[i]
                if y_t[i] > u_t[i]:
                    y_t[i] = u_t[i]
            f = f32(cost_of(inv(y_t)))
            nfg += 1
            if f < gx:
                gx, jfaa, x_t = f, 0, y_t.copy()
                x = inv(x_t)
                events.add("line_accepted")
                if gx < f32(ga - f32(2)):
                    ga = gx
            else:
                events.add("line_rejected")
        ia = 0
        if it % n == 0:
            rows.append((gx, x.copy(), nfg, ddx))
        if ddx < f32(0.01):
            msg = "CONVERGENCE: DDX < 0.01"; break
        if it == maxiter * n:
            msg = "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT"; break
    return rows, msg, events, (gx, x.copy(), nfg, it if maxiter * n else 0)


NOISE_SEEDS = 6


def at(rows, last, n, k):
    """(cost, x) after a run of maxiter = k: iterate k, or the point at which the run ended before it"""
    return (rows[k][0], rows[k][1]) if k < len(rows) and k * n <= last[3] else (last[0], last[1])


def bars_ratio(got, cs_ref, xs_ref):
    """the worst deviation of a trajectory [(cost, x)] from the recorded one in units of the bars the default build is held to"""
    worst = abs(float(got[0][0]) - float(cs_ref[0])) / (3e-7 + 1e-5 * abs(float(cs_ref[0])))
    for k in range(1, len(cs_ref)):
        worst = max(worst, abs(float(got[k][0]) - float(cs_ref[k])) / (0.02 * abs(float(cs_ref[k]))))
        for a, b in zip(got[k][1], xs_ref[k]):
            worst = max(worst, abs(float(a) - float(b)) / (0.02 * abs(float(b)) + 1e-3))
    return worst


def problem(fx):
    """the case with the start point written over the whole grid, and the options of the run"""
    import golden_util as gu
    from smash_amd.synth import PARAM_NAMES, STATE_NAMES
    g = gu.load(fx["case"])
    P = {k: v.copy(order="F") for k, v in g.params.items()}
    S = {k: v.copy(order="F") for k, v in g.states.items()}
    for k, v in zip(fx["fields"], fx["x0"]):
        (P if k in P else S)[k][:] = f32(v)
    op = np.array([1 if k in fx["fields"] else 0 for k in PARAM_NAMES], np.int32)
    os_ = np.array([1 if k in fx["fields"] else 0 for k in STATE_NAMES], np.int32)
    from smash_amd import types as T
    lbp, ubp, lbs, ubs = T.GLB_PARAMETERS.copy(), T.GUB_PARAMETERS.copy(), T.GLB_STATES.copy(), T.GUB_STATES.copy()
    for k, lo, hi in zip(fx["fields"], fx["lb"], fx["ub"]):
        if k in PARAM_NAMES:
            lbp[PARAM_NAMES.index(k)], ubp[PARAM_NAMES.index(k)] = lo, hi
        else:
            lbs[STATE_NAMES.index(k)], ubs[STATE_NAMES.index(k)] = lo, hi
    # the control vector in stacked order
    order = [k for k in tuple(PARAM_NAMES) + tuple(STATE_NAMES) if k in fx["fields"]]
    opts = dict(g.opts, optim_parameters=op, optim_states=os_, lb_parameters=lbp, ub_parameters=ubp, lb_states=lbs, ub_states=ubs)
    return g, P, S, order, opts


def cost_function(g, P, S, order, opts, run):
    act = np.asarray(g.mesh.active_cell) == 1
    plain = {k: v for k, v in opts.items() if not k.startswith(("optim_", "lb_", "ub_"))}

    def cost_of(y):
        p = {k: v.copy(order="F") for k, v in P.items()}
        s = {k: v.copy(order="F") for k, v in S.items()}
        for k, v in zip(order, y):
            (p if k in p else s)[k][act] = f32(v)
        return f32(run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, p, s, **plain)["cost"])
    return cost_of


def record(name, fx, write=True):
    from oracle import pyoracle, refbind
    g, P, S, order, opts = problem(fx)
    pos = {k: i for i, k in enumerate(fx["fields"])}
    l = [fx["lb"][pos[k]] for k in order]
    u = [fx["ub"][pos[k]] for k in order]
    x0 = [fx["x0"][pos[k]] for k in order]
    cost_of = cost_function(g, P, S, order, opts, pyoracle.run)
    K = fx["K"]
    rows, msg, events, last = sbs_restated(cost_of, x0, l, u, K, cost_of(np.array(x0, f32)))
    print(f"{name}: restated {len(rows) - 1} iterates, '{msg}', nfg {last[2]}, inner iterations {last[3]}, events {sorted(events)}")
    missing = [e for e in fx["needs"] if e not in events]
    if missing or not msg.startswith(fx["stop"]):
        raise SystemExit(f"{name}: refused, the run lacks {missing} or does not end by {fx['stop']} ('{msg}')")
    act = np.asarray(g.mesh.active_cell) == 1
    first = int(np.argmax(act.reshape(-1, order="F")))
    r0, c0 = first % g.mesh.nrow, first // g.mesh.nrow
    costs, xs = [], []
    for k in range(K + 1):
        r = refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, P, S, optimize_sbs_maxiter=k, **opts)
        costs.append(f32(r["cost"]))
        xs.append(np.array([(r["parameters"] if f in r["parameters"] else r["states"])[f][r0, c0] for f in order], f32))
    # the restatement against the reference: iterate k while the run lasts, the final point afterwards (a run that converged at an
    # iteration that is no multiple of n has no row for it)
    for k in range(K + 1):
        want = rows[k] if k < len(rows) and not (msg.startswith("CONVERGENCE") and k == len(rows) - 1 and last[3] % len(order)) else (last[0], last[1])
        if k >= len(rows):
            want = (last[0], last[1])
        if k == 0:
            want = (rows[0][0], np.array(x0, f32))
        if f32(want[0]).tobytes() != costs[k].tobytes() or np.asarray(want[1], f32).tobytes() != xs[k].tobytes():
            raise SystemExit(f"{name}: refused, the restatement leaves the reference at k = {k}: {want[0]} {want[1]} vs {costs[k]} {xs[k]}")
    fast_ratio = noise_ratio = -1.0
    if fx["needs"] == ALL:
        n = len(order)
        fast = []
        for k in range(K + 1):
            r = refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, P, S, optimize_sbs_maxiter=k, fast=True, **opts)
            fast.append((f32(r["cost"]), [(r["parameters"] if f in r["parameters"] else r["states"])[f][r0, c0] for f in order]))
        fast_ratio = bars_ratio(fast, costs, xs)
        noise_ratio = 0.0
        for seed in range(NOISE_SEEDS):
            rng, pert = np.random.default_rng(100 + seed), {}

            def noisy(y):
                key = np.asarray(y, f32).tobytes()
                if key not in pert:
                    pert[key] = f32(float(cost_of(y)) * (1.0 + g.noise["cost"] * rng.uniform(-1, 1)))
                return pert[key]
            rr, _, _, ll = sbs_restated(noisy, x0, l, u, K, noisy(np.array(x0, f32)))
            noise_ratio = max(noise_ratio, bars_ratio([at(rr, ll, n, k) for k in range(K + 1)], costs, xs))
        print(f"{name}: the reference's other build stays within {fast_ratio:.3f} of the bars, the noise-perturbed restatement within {noise_ratio:.3f}")
        if not (fast_ratio <= 1.0 and noise_ratio <= 1.0):
            raise SystemExit(f"{name}: refused, the reference's own error moves the trajectory past the bars")
    d = dict(case=fx["case"], fast_ratio=fast_ratio, noise_ratio=noise_ratio, fields=np.array(order), lb=np.array(l, f32), ub=np.array(u, f32), x0=np.array(x0, f32), K=K,
             cost=np.array(costs, f32), x=np.stack(xs), nfg=np.array([r[2] for r in rows], np.int32), ddx=np.array([r[3] for r in rows], f32),
             task=msg, inner_iterations=last[3], nfg_total=last[2], events=np.array(sorted(events)))
    if write:
        os.makedirs(OUT, exist_ok=True)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"{name}: costs {[float(c) for c in costs]}")
    return d


if __name__ == "__main__":
    for name in (sys.argv[1:] or FIXTURES):
        record(name, FIXTURES[name])
