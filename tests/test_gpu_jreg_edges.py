"""GPU: the regularisation term of the cost (compute_jreg: smash_amd/csrc/sx_jreg.h, run_jreg / seed_gradients / the download of
inactive cells and unused fields / the jreg_d part of smashx_forward_d in smashx.hip) at the edges of grid shape, mask and sum
length: the cases of tests/jreg_cases.py (nrow != ncol, holes, one-cell strips, isolated cells, one row, one column; running sums of
0, 9 .. 63, 64, 65, 255, 256, 257, 320, 512, 513 terms; njr = 4, eight sums), each with the default gauge weights ("w") and with
every gauge weight zero ("z").  Reference: the plain-C oracle, which tests/test_jreg_edges_cpu.py pins to the compiled reference bit
for bit on exactly these cases.  Forward, adjoint and tangent through smash_amd.forward / forward_b / forward_d.

EQUAL FP32 BITS IN BOTH BUILDS (no libm on these paths; sx_jreg.h sums in the reference's order):
  * cost_jreg after forward, after forward_b and after forward_d (the last one: the sums are put back after the tangent reused them);
  * jreg_d (Solver.tangent_terms()[1]): in "z" cost_d is the oracle's cost_d and jobs_d is 0; in "w" jreg_d equals the "z" run's;
  * "z" without an optimised state (jreg_cases.NO_STATE): all 24 gradient planes and cost = wjreg * cost_jreg.  (With an optimised
    state the regulariser's gradient seeds that state's adjoint in the sweep and passes through libm.)
  * always: every gradient plane on the inactive cells, and the whole plane of the fields gr-b does not use.
SWEEP-DEPENDENT OUTPUTS (discharge, cost, final states, the gradient on active cells, qsim_d, cost_d) by the unchanged rule of
tests/test_gpu_parity_at_size._check: the exact-libm build bit-identical to the fp32 oracle (tangent outputs excepted, as there), the
default build e_hip <= 2 e_ref + 1e-6 against the fp64 oracle, costs |hip - truth| <= 2 |ref - truth| + 3e-7.
test_exact_build_runs_this_file re-runs the file under SMASHX_EXACT_LIBM=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import jreg_cases as jc
from smash_amd import synth
from test_gpu_parity import _types
from test_gpu_parity_at_size import _check

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = [(cid, w) for cid in jc.IDS for w in jc.WEIGHTINGS]
FIELDS = tuple(synth.PARAM_NAMES) + tuple(synth.STATE_NAMES)
USED = gu.STRUCT_PARAMS[jc.STRUCTURE] + gu.STRUCT_STATES[jc.STRUCTURE]
F32 = np.float32

_runs = {}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64), F32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _adjoint(g, inp_types=None, params=None, states=None):
    """One adjoint sweep of case g (on the (setup, mesh, inp, ...) of an earlier _types call when given: the same Solver; with other
    field values when given): cost, cost_jreg and the 24 gradient planes."""
    import smash_amd
    setup, mesh, inp, par, sta, o = inp_types or _types(g)
    if params is not None:
        par, sta = smash_amd.ParametersDT.from_dict(mesh, params), smash_amd.StatesDT.from_dict(mesh, states)
    else:
        par, sta = smash_amd.ParametersDT.from_dict(mesh, g.params), smash_amd.StatesDT.from_dict(mesh, g.states)
    par_b, sta_b = par.copy(), sta.copy()              # (not zero: forward_b overwrites every plane)
    smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), o, o.copy(),
                        F32(0), F32(1))
    out = {"adj.cost": o.cost, "adj.cost_jreg": o.cost_jreg, "adj.qsim": o.qsim.copy()}
    out.update({k + "_b": getattr(par_b, k).copy() for k in synth.PARAM_NAMES})
    out.update({k + "_b": getattr(sta_b, k).copy() for k in synth.STATE_NAMES})
    return out


def _tangent(g, inp_types=None):
    """One tangent sweep along g.direction (parameters and states): qsim_d, cost_d, cost_jreg and (jobs_d, jreg_d)."""
    import smash_amd
    setup, mesh, inp, par, sta, o = inp_types or _types(g)
    par_d, sta_d = smash_amd.ParametersDT.from_dict(mesh, g.direction[0]), smash_amd.StatesDT.from_dict(mesh, g.direction[1])
    o_d = smash_amd.OutputDT(setup, mesh)
    _, cost_d = smash_amd.forward_d(setup, mesh, inp, par, par_d, inp._bgd[0], par.copy(), sta, sta_d, inp._bgd[1], sta.copy(), o, o_d)
    return {"qsim_d": o_d.qsim.copy(), "cost_d": cost_d, "tan.cost_jreg": o.cost_jreg, "tan.terms": inp._smashx_solver.tangent_terms()}


def _forward(g):
    import smash_amd
    setup, mesh, inp, par, sta, o = _types(g)
    smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], o, F32(0))
    out = {"qsim": o.qsim.copy(), "cost": o.cost, "cost_jreg": o.cost_jreg}
    out.update({"fstates." + k: getattr(o.fstates, k).copy() for k in gu.STRUCT_STATES[g.structure]})
    return out


def _run(cid, w):
    """(case, GPU outputs of the three sweeps -- each through a Solver of its own --, {False: fp32 oracle, True: fp64 oracle}); once"""
    if (cid, w) not in _runs:
        g = jc.build(cid, w)
        hip = dict(_forward(g), **_adjoint(g), **_tangent(g))
        _runs[cid, w] = (g, hip, {f64: jc.oracle_outputs(g, fp64=f64) for f64 in (False, True)})
    return _runs[cid, w]


@pytest.mark.parametrize("cid,w", CASES)
def test_regulariser_at_the_edges_vs_oracle(cid, w):
    g, hip, ref = _run(cid, w)
    o32 = ref[False]
    act = np.asarray(g.mesh.active_cell) == 1
    op, os_ = jc.optimised(cid)
    optim = {k for k, f in zip(FIELDS, list(op) + list(os_)) if f}
    bad = []
    # --- the regulariser's value: after each of the three sweeps
    print(f"{cid}.{w} cost_jreg hip {hip['cost_jreg']!r} / {hip['adj.cost_jreg']!r} / {hip['tan.cost_jreg']!r} oracle {float(o32['cost_jreg'])!r}"
          f"   jobs_d, jreg_d {hip['tan.terms']}  cost_d hip {hip['cost_d']!r} oracle {float(o32['cost_d'])!r}")
    bad += [k for k in ("cost_jreg", "adj.cost_jreg", "tan.cost_jreg") if not _same(hip[k], o32["cost_jreg"])]
    assert _same(o32["adj.cost_jreg"], o32["cost_jreg"])
    # --- its tangent
    if w == "z":
        if not _same(hip["cost_d"], o32["cost_d"]):
            bad.append("cost_d (z)")
        if hip["tan.terms"][0] != 0.0:
            bad.append("jobs_d (z)")
        if not _same(hip["cost_d"], F32(jc.JREG["wjreg"]) * F32(hip["tan.terms"][1])):
            bad.append("cost_d = wjreg jreg_d")
    # --- its gradient where nothing else enters (reg_prior sums over the whole grid: not zero on the inactive cells of a mask)
    if cid in jc.MASKED:
        assert all(np.any(o32[k + "_b"][~act]) for k in optim - {"ci"}), "the reference's gradient on inactive cells is zero"
    for k in FIELDS:
        a, b = hip[k + "_b"], o32[k + "_b"]
        if not _same(a[~act], b[~act]):
            bad.append(k + "_b on inactive cells")
        if k not in USED:
            if not _same(a, b):
                bad.append(k + "_b (unused field)")
            if k not in optim and (np.any(a) or np.any(b)):
                bad.append(k + "_b (unused, never optimised) is not zero")
        if w == "z" and cid in jc.NO_STATE and not _same(a, b):
            bad.append(k + "_b (the regulariser's alone)")
    if w == "z" and cid in jc.NO_STATE:
        for k in ("cost", "adj.cost"):
            if not (_same(hip[k], o32[k]) and _same(hip[k], F32(jc.JREG["wjreg"]) * F32(hip["cost_jreg"]))):
                bad.append(k + " = wjreg cost_jreg")
        assert any(np.any(hip[k + "_b"]) for k in optim)
    # --- everything the sweep touches, by the rule of the at-size tests
    sweep = {k: hip[k] for k in ("qsim", "cost", "adj.cost", "qsim_d", "cost_d")}
    sweep.update({k: v for k, v in hip.items() if k.startswith("fstates.")})
    sweep.update({k + "_b": hip[k + "_b"] for k in USED})
    bad += _check(f"{cid}.{w}", sweep, ref)
    assert not bad, (cid, w, bad)


@pytest.mark.parametrize("cid", jc.IDS)
def test_jreg_d_does_not_depend_on_the_gauge_weights(cid):
    """the oracle returns no jreg_d of its own: the "z" run's is held to the oracle's cost_d above, the "w" run's to the "z" run's"""
    tw, tz = _run(cid, "w")[1]["tan.terms"], _run(cid, "z")[1]["tan.terms"]
    print(f"{cid}: (jobs_d, jreg_d) w {tw} z {tz}")
    assert _same(tw[1], tz[1]) and tz[1] != 0.0


def test_checkerboard_leaves_the_priors_alone():
    """checker_6x11: every 4-neighbour of an active cell is inactive, so every smoothing term is (m0 - 2 m0 + m0)^2 = 0 and both
    smoothing sums are exactly 0; cost_jreg is what the two priors alone give (adding + 0 changes no running sum)."""
    import smash_amd
    g, hip, ref = _run("checker_6x11", "z")
    got = {}
    for name, funs, ws in (("smoothing", ("smoothing", "hard_smoothing"), (0.5, 0.1)), ("priors", ("prior", "prior"), (1.0, 0.25))):
        h = jc.build("checker_6x11", "z", qobs=g.qobs)
        h.opts.update(jreg_fun=funs, wjreg_fun=ws)
        setup, mesh, inp, par, sta, o = _types(h)
        par_b, sta_b = par.copy(), sta.copy()
        smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), o, o.copy(), F32(0), F32(1))
        got[name] = (o.cost_jreg, {k: getattr(par_b if k in synth.PARAM_NAMES else sta_b, k).copy() for k in FIELDS})
    assert got["smoothing"][0] == 0.0 and not any(np.any(v) for v in got["smoothing"][1].values()), got["smoothing"][0]
    assert got["priors"][0] != 0.0 and _same(got["priors"][0], hip["cost_jreg"]) and _same(hip["cost_jreg"], ref[False]["cost_jreg"])
    for k in FIELDS:                                   # and the gradient is the priors' gradient
        assert _same(got["priors"][1][k], hip[k + "_b"]), k


def _other_fields(g):
    """field values halfway to the background: another control vector for the same case"""
    mid = lambda a, b: {k: np.asfortranarray((F32(0.5) * (a[k] + b[k])).astype(F32)) for k in a}
    return mid(g.params, g.opts["params_bgd"]), mid(g.states, g.opts["states_bgd"])


@pytest.mark.parametrize("w", jc.WEIGHTINGS)
def test_second_adjoint_sweep_of_a_solver_carries_nothing_over(w):
    """holes_7x19, two adjoint sweeps through one Solver with different field values: the second equals a fresh Solver's (the
    regulariser's gradient planes are zeroed again, the sums and the seeds are those of the second control vector)"""
    g, hip, _ = _run("holes_7x19", w)
    t = _types(g)
    p2, s2 = _other_fields(g)
    first = _adjoint(g, t, p2, s2)
    second = _adjoint(g, t)
    assert t[2]._smashx_solver is not None
    assert not _same(first["adj.cost_jreg"], second["adj.cost_jreg"]) and not _same(first["cp_b"], second["cp_b"])
    bad = [k for k in second if not _same(second[k], hip[k])]
    assert not bad, bad


@pytest.mark.parametrize("w", jc.WEIGHTINGS)
def test_adjoint_after_tangent_on_one_solver(w):
    """holes_7x19, forward_d then forward_b on one Solver (the tangent reuses the term planes and the sums of the regulariser):
    forward_b's outputs equal a fresh Solver's"""
    g, hip, _ = _run("holes_7x19", w)
    t = _types(g)
    tan = _tangent(g, t)
    s = t[2]._smashx_solver
    adj = _adjoint(g, t)
    assert t[2]._smashx_solver is s
    assert _same(tan["cost_d"], hip["cost_d"]) and _same(tan["tan.cost_jreg"], hip["cost_jreg"])
    bad = [k for k in adj if not _same(adj[k], hip[k])]
    assert not bad, bad


N_TESTS = len(CASES) + len(jc.IDS) + 1 + 2 * len(jc.WEIGHTINGS)


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    sys.stdout.write(r.stdout[-8000:])
    assert r.returncode == 0 and f"{N_TESTS} passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
