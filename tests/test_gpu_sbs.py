"""GPU: smash_amd.optimize_sbs, the mirror of the reference's uniform step-by-step calibration, over its three cost routes (the
catchment-resident kernel, the ensemble, the loop of forwards) and against the reference's own runs: tests/golden/sbs/ (the cost and
the calibrated values after every iteration, tests/golden/make_sbs.py) and tests/golden/lbfgsb/sbs_gr_a_cance.npz (the user guide's
first calibration).  Every case runs in the build the session selects; test_exact_build_runs_this_file re-runs the file under
SMASHX_EXACT_LIBM=1, where the trajectory is the reference's bit for bit.  The default build is held to the bars of
tests/test_gpu_dropin.py::test_reference_sbs_on_cance_through_dropin."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import golden_util as gu
from test_gpu_parity import _types

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_sbs as ms  # noqa: E402

FULL = ("gr_b_16x16x96_nse_gaps", "gr_a_12x12x48_nse")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _fixture_problem(name):
    z = np.load(os.path.join(gu.GOLDEN_DIR, "sbs", name + ".npz"))
    fx = dict(case=str(z["case"]), fields=tuple(str(k) for k in z["fields"]), lb=tuple(z["lb"]), ub=tuple(z["ub"]), x0=tuple(z["x0"]), K=int(z["K"]))
    g, P, S, order, opts = ms.problem(fx)
    h = types.SimpleNamespace(**vars(g))
    h.params, h.states, h.opts = P, S, {k: v for k, v in opts.items() if not k.startswith(("lb_", "ub_"))}
    setup, mesh, inp, par, sta, out = _types(h)
    o = setup.optimize
    o.lb_parameters, o.ub_parameters, o.lb_states, o.ub_states = (opts[k].copy() for k in ("lb_parameters", "ub_parameters", "lb_states", "ub_states"))
    o.maxiter = fx["K"]
    return z, fx, (setup, mesh, inp, par, sta, out)


_runs = {}


def _run(name, route):
    """one calibration per (fixture, route), shared by the tests below"""
    import smash_amd
    if (name, route) not in _runs:
        z, fx, (setup, mesh, inp, par, sta, out) = _fixture_problem(name)
        hist = smash_amd.optimize_sbs(setup, mesh, inp, par, sta, out, candidates=route)
        _runs[(name, route)] = (z, fx, hist, (setup, mesh, inp, par, sta, out))
    return _runs[(name, route)]


def _same_trajectory(a, b):
    return (np.array_equal(_bits(a["cost"]), _bits(b["cost"])) and np.array_equal(_bits(np.stack(a["x"])), _bits(np.stack(b["x"])))
            and a["nfg"] == b["nfg"] and np.array_equal(_bits(a["ddx"]), _bits(b["ddx"])) and a["task"] == b["task"] and a["iter"] == b["iter"]
            and _bits(a["final_cost"]) == _bits(b["final_cost"]) and np.array_equal(_bits(a["final_x"]), _bits(b["final_x"])))


@pytest.mark.parametrize("name", FULL)
def test_the_three_routes_give_one_trajectory(name):
    res, ens, loop = (_run(name, r)[2] for r in ("resident", "ensemble", "loop"))
    print(name, "costs", res["cost"], res["task"], "nfg", res["nfg_total"])
    assert len(res["cost"]) > 3
    assert _same_trajectory(res, loop) and _same_trajectory(ens, loop)
    assert _same_trajectory(_run(name, "auto")[2], loop) and _run(name, "auto")[2]["route"] == "auto"


@pytest.mark.parametrize("name", sorted(ms.FIXTURES))
def test_trajectory_against_the_reference(name):
    """Exact-libm build: the reference's trajectory bit for bit, all four fixtures.  Default build: the drop-in test's bars (first cost
    3e-7 + 1e-5 |ref|, later costs 2 %, values 2 % + 1e-3).  The optimiser's `f < gx` is a discontinuous function of costs that differ from
    the reference's in their last bits, so the recorder only keeps a full fixture that the reference's own other build and the
    reference's own cost noise follow within these bars (tests/golden/make_sbs.py)."""
    from smash_amd import _lib
    z, fx, hist, _ = _run(name, "resident")
    n, K = len(fx["x0"]), fx["K"]
    rows = [(hist["cost"][k], hist["x"][k]) if k < len(hist["cost"]) and k * n <= hist["iter"] else (hist["final_cost"], hist["final_x"]) for k in range(K + 1)]
    for k, (c, x) in enumerate(rows):
        print(f"{name} k={k}: cost {c!r} vs {float(z['cost'][k])!r}, x {x} vs {z['x'][k]}")
    if _lib.EXACT:
        for k, (c, x) in enumerate(rows):
            assert _bits(c) == _bits(z["cost"][k]) and np.array_equal(_bits(x), _bits(z["x"][k])), k
        assert hist["task"] == str(z["task"]) and hist["iter"] == int(z["inner_iterations"]) and hist["nfg_total"] == int(z["nfg_total"])
        assert hist["nfg"] == list(z["nfg"])
        return
    ref = z["cost"]
    assert abs(rows[0][0] - ref[0]) <= 3e-7 + 1e-5 * abs(ref[0]), (rows[0][0], ref[0])
    for k in range(1, K + 1):
        assert abs(rows[k][0] - ref[k]) <= 0.02 * abs(ref[k]), (k, rows[k][0], ref[k])
        for i in range(n):
            assert abs(float(rows[k][1][i]) - float(z["x"][k][i])) <= 0.02 * abs(float(z["x"][k][i])) + 1e-3, (k, i, rows[k][1], z["x"][k])


def _cance(jobs=None):
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "sbs_gr_a_cance.npz"))
    g = gu.load("gr_a_cance_28x28x1440")
    pv = dict(ci=1e-6, cp=200.0, beta=1000.0, cft=500.0, cst=500.0, alpha=0.9, exc=0.0, lr=5.0)
    h = types.SimpleNamespace(**vars(g))
    h.params = {k: (np.full_like(v, pv[k]) if k in pv else v) for k, v in g.params.items()}
    setup, mesh, inp, par, sta, out = _types(h)
    setup.optimize.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
    setup.optimize.optim_states = np.zeros(8, np.int32)
    if jobs:
        setup.optimize.jobs_fun, setup.optimize.wjobs_fun = list(jobs), [1.0 / len(jobs)] * len(jobs)
        inp.mean_prcp = np.asfortranarray(np.load(os.path.join(gu.GOLDEN_DIR, "mean_forcing", "gr_a_cance_28x28x1440.npz"))["mean_prcp"])
    return z, (setup, mesh, inp, par, sta, out)


def test_cance_and_what_optimize_sbs_leaves_behind():
    """the user guide's first calibration (cp, cft, exc, lr from the Model() defaults, maxiter 2) against the all-CPU reference; then
    the state the call leaves: values on the active cells only, output = a forward at the returned fields"""
    import smash_amd
    z, (setup, mesh, inp, par, sta, out) = _cance()
    setup.optimize.maxiter = 2
    act = np.asarray(mesh.active_cell) == 1
    assert 0 < act.sum() < act.size
    par.cp[~act], par.lr[~act] = f32(-7.0), f32(-8.0)              # inactive cells keep what they hold
    keep_cst = par.cst.copy()
    hist = smash_amd.optimize_sbs(setup, mesh, inp, par, sta, out, candidates="auto")
    costs, ref = hist["cost"], z["costs"]
    print("cance sbs:", costs, "reference", ref, hist["task"], "nfg", hist["nfg"], "route", hist["route"])
    assert len(costs) == 3 and hist["route"] == "auto"
    assert abs(costs[0] - ref[0]) <= 3e-7 + 1e-5 * abs(ref[0]), (costs, ref)
    for a, b in zip(costs[1:], ref[1:]):
        assert abs(a - b) <= 0.02 * abs(b), (costs, ref)
    fields = ("cp", "cft", "exc", "lr")
    for i, k in enumerate(fields):
        v = getattr(par, k)
        assert abs(float(v[20, 27]) - float(z["final_" + k])) <= 0.02 * abs(float(z["final_" + k])) + 1e-3, k
        assert np.all(_bits(v[act]) == _bits(hist["final_x"][i])), k
    assert np.all(par.cp[~act] == f32(-7.0)) and np.all(par.lr[~act] == f32(-8.0)) and np.array_equal(_bits(par.cst), _bits(keep_cst))
    assert hist["fields"] == list(fields) and hist["task"] == "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT"
    assert _bits(out.cost) == _bits(hist["final_cost"]) == _bits(costs[2])
    o2 = smash_amd.OutputDT(setup, mesh)
    smash_amd.forward(setup, mesh, inp, par, par.copy(), sta, sta.copy(), o2, f32(0))
    assert _bits(o2.cost) == _bits(out.cost) and np.array_equal(_bits(o2.qsim), _bits(out.qsim))


def test_a_signature_criterion_runs_through_auto():
    """("nse", "Crc"): smashx_uniform_costs refuses the options, "auto" falls back to the loop of forwards and says so"""
    import smash_amd
    hists = []
    for route in ("auto", "loop"):
        z, (setup, mesh, inp, par, sta, out) = _cance(jobs=("nse", "Crc"))
        setup.optimize.maxiter = 1
        hists.append(smash_amd.optimize_sbs(setup, mesh, inp, par, sta, out, candidates=route))
    print("cance nse + Crc:", hists[0]["cost"], hists[0]["route"])
    assert hists[0]["route"].startswith("auto -> loop") and "signature" in hists[0]["route"]
    assert len(hists[0]["cost"]) == 2 and hists[0]["cost"][1] < hists[0]["cost"][0]
    assert _same_trajectory(hists[0], hists[1])
    with pytest.raises(smash_amd.SmashxError):
        z, (setup, mesh, inp, par, sta, out) = _cance(jobs=("nse", "Crc"))
        setup.optimize.maxiter = 1
        smash_amd.optimize_sbs(setup, mesh, inp, par, sta, out, candidates="resident")


def test_verbose_prints_the_iterate_lines(capsys):
    import smash_amd
    z, fx, (setup, mesh, inp, par, sta, out) = _fixture_problem("gr_b_16x16x96_nse_gaps_maxiter")
    hist = smash_amd.optimize_sbs(setup, mesh, inp, par, sta, out, verbose=True)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert lines[0] == f"    At iterate      0    nfg =     1    J ={hist['cost'][0]:10.6f}    ddx = 0.64"
    assert lines[2].startswith("    At iterate      2    nfg = ") and lines[-1] == "    STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT"


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=1500, cwd=ROOT)
    sys.stdout.write(r.stdout[-8000:])
    assert r.returncode == 0 and "9 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
