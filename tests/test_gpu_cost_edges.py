"""GPU: the gauge cost stage (smash_amd/csrc/sx_cost.h: sx_k_cost_sums, sx_k_cost_final, sx_k_cost_seeds, sx_k_cost_cellseeds,
sx_k_cost_tangent) at its edges -- the cases of tests/cost_edge_cases.py: windows of 1 .. 200 steps around the 64-step loads, start
steps 0, 5, 63, 64 and nt - 1, missing data, zero, equal and constant series, values spanning nine decades, each criterion alone and
eight at once, 1 .. 70 gauges, zero weights, the median over 1 .. 65 gauges with and without ties, and gauges without data.

FUNCTION LEVEL.  Every recorded case runs through Solver.jobs_of_qsim (compute_jobs / _B / _D on a prescribed discharge) against
what the compiled reference recorded (tests/golden/cost_edges/cost_edges.npz), for the seeds jobs_b = 1 and 2.5.
  * nse, kge, kge2, se, rmse, their mixes, the gauge weighting and the median hold only correctly rounded + - x / sqrt and the build is
    -O3 -ffp-contract=off without fast-math: jobs, qsim_b and jobs_d equal the reference's fp32 BITS (or are NaN where it is NaN) in
    BOTH builds of the library.
  * cases with `logarithmic`: bit for bit in the exact-libm build; in the default build by the unchanged rule of
    tests/test_gpu_parity_at_size._check against the fp64 restatement as truth (cost |hip - truth| <= 2 |ref - truth| + 3e-7, seeds
    e_hip <= 2 e_ref + 1e-6), on the entries where the reference is finite; where it is not, the same NaN / Inf is required.
  * always: qsim_b is exactly 0 before the start step, on missing steps, on zero-weight gauges and on positive-weight gauges under a
    median.
STATE.  jobs_of_qsim leaves the last sweep's gauge discharges and cost as they were; a second call with fewer criteria does not see
the coefficients of the first.
GAUGES WITHOUT DATA (non-zero weight, no qobs >= 0 from the start step on) count as weight 0: jobs_of_qsim, forward / forward_b /
forward_d, multiple_run and uniform_costs with the gauge weighted equal the run with its weight set to 0 bit for bit; on a plan with
median slots such a gauge is refused by the call that completes (options, qobs), and one observation brings it back.
TWO GAUGES ON ONE CELL: a whole sweep against the oracle by _check's rule.
test_exact_build_runs_this_file re-runs the file under SMASHX_EXACT_LIBM=1."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import cost_edge_cases as ce
import golden_util as gu
import jreg_cases as jc
import multiple_run_util as mu
from test_gpu_jreg_edges import _adjoint, _forward, _tangent
from test_gpu_parity import _types
from test_gpu_parity_at_size import _check

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32
FIX = ce.load_fixture()
EMPTY = ce.empty_cases()


def _exact():
    from smash_amd import _lib
    return _lib.EXACT


# ---- function level --------------------------------------------------------------------------------------------------------------------
_plans = {}


def _plan(r, nt):
    """a plan over the 12 x 12 mesh with the gauges of record r (gauge_pos, area), dt = 3600, dx = 500; shared by the cases that agree"""
    import smash_amd
    from smash_amd.solver import Solver
    key = (nt, r["gauge_pos"].tobytes(), r["area"].tobytes())
    if key not in _plans:
        m = ce.base_mesh()
        ng = r["area"].size
        setup = smash_amd.SetupDT(0, ng, structure="gr-a", dt=ce.DT, ntime_step=nt)
        mesh = smash_amd.MeshDT(setup, m.nrow, m.ncol, ng)
        mesh.dx = ce.DX
        mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.flwdir, m.flwacc, m.path, m.active_cell
        mesh.gauge_pos = np.asfortranarray(r["gauge_pos"].astype(np.int32))
        mesh.area = np.ascontiguousarray(r["area"], F32)
        _plans[key] = (setup, Solver(setup, mesh))
    return _plans[key]


def _probe(r, jobs_fun=None, wjobs=None, wgauge=None, qobs=None, plan=None):
    """jobs_of_qsim on record / case r for both seeds: (jobs, jobs_d, qsim_b for JOBS_B[0], qsim_b for JOBS_B[1])"""
    qobs = r["qobs"] if qobs is None else qobs
    setup, s = plan or _plan(r, qobs.shape[1])
    s.set_qobs(np.asfortranarray(qobs, F32))
    o = setup.optimize
    o.jobs_fun = list(r["jobs_fun"] if jobs_fun is None else jobs_fun)
    o.wjobs_fun = [float(w) for w in (r["wjobs"] if wjobs is None else wjobs)]
    o.optimize_start_step, o.wgauge = int(r["start"]), np.asarray(r["wgauge"] if wgauge is None else wgauge, F32)
    s.set_options(o)
    qsim, qsim_d = np.asfortranarray(r["qsim"], F32), np.asfortranarray(r["qsim_d"], F32)
    j1, b1, d1 = s.jobs_of_qsim(qsim, jobs_b=ce.JOBS_B[0], qsim_d=qsim_d)
    j2, b2, d2 = s.jobs_of_qsim(qsim, jobs_b=ce.JOBS_B[1], qsim_d=qsim_d)
    assert ce.same_bits(j1, j2) and ce.same_bits(d1, d2)
    return j1, d1, b1, b2


def _exact_zeros(r, b):
    """where no seed may land"""
    s0 = r["start"] - 1
    qo = ce.normalised(dict(r, ng=r["area"].size, nt=r["qobs"].shape[1]))[0]
    w = r["wgauge"]
    bad = []
    if b[:, :s0].any():
        bad.append("before the start step")
    if b[:, s0:][~(qo[:, s0:] >= 0)].any():
        bad.append("on missing steps")
    if b[w == 0].any():
        bad.append("on zero-weight gauges")
    if np.any(w < 0) and b[w > 0].any():
        bad.append("on positive-weight gauges under a median")
    return bad


def _finite_part(a, *masks):
    a = np.array(a, np.float64)
    keep = np.ones(a.shape, bool)
    for m in masks:
        keep &= np.isfinite(np.asarray(m, np.float64))
    return np.where(keep, a, 0.0), keep


@pytest.mark.parametrize("name", list(FIX))
def test_recorded_cases_through_jobs_of_qsim(name):
    r = FIX[name]
    jobs, jobs_d, b1, b2 = _probe(r)
    got = {"jobs": jobs, "jobs_d": jobs_d, "qsim_b1": b1, "qsim_b2": b2}
    differ = [k for k in got if not ce.same_bits(got[k], r[k])]
    print(f"{name} {'exact-libm' if _exact() else 'default'}: jobs {jobs!r} (reference {r['jobs']!r}) jobs_d {jobs_d!r} ({r['jobs_d']!r}); differing: {differ}")
    bad = _exact_zeros(r, b1) + _exact_zeros(r, b2)
    if "logarithmic" not in r["jobs_fun"] or _exact():
        bad += differ
    else:
        c = ce.cases()[name]
        hip, ref = {}, {False: {}, True: {}}
        for jb, key in zip(ce.JOBS_B, ("qsim_b1", "qsim_b2")):
            t = ce.restate(c, np.float64, jobs_b=jb)
            for k, h, r32, t64 in (("cost", jobs, r["jobs"], t["jobs"]), ("cost_d", jobs_d, r["jobs_d"], t["jobs_d"]), (key, got[key], r[key], t["qsim_b"])):
                r0, keep = _finite_part(r32, r32, t64)
                if not ce.same_bits(np.asarray(h, F32)[~keep], np.asarray(r32, F32)[~keep]):
                    bad.append(k + ": not the reference's NaN / Inf")
                if k in ("cost", "cost_d"):
                    if keep:
                        hip[k], ref[False][k], ref[True][k] = float(h), np.float64(r32), np.float64(t64)
                else:
                    hip[k], ref[False][k], ref[True][k] = _finite_part(h, r32, t64)[0], r0, _finite_part(t64, r32, t64)[0]
                    assert np.isfinite(np.asarray(h)[keep]).all()
        bad += _check(name, hip, ref)
        for k in hip:              # the figures DESIGN.md section 5 quotes
            den = np.sqrt(np.sum(np.square(ref[False][k]))) or 1.0
            print(f"  {name} {k}: |hip - reference| / |reference| = {np.sqrt(np.sum(np.square(np.asarray(hip[k], np.float64) - ref[False][k]))) / den:.3e}")
    assert not bad, (name, bad)


# ---- state -------------------------------------------------------------------------------------------------------------------------------
def test_probe_leaves_the_last_sweep_alone():
    """a forward sweep of a three-gauge golden input, then jobs_of_qsim on another discharge: the plan's gauge discharges and cost
    read back as the sweep left them"""
    import smash_amd
    g = gu.load("gr_b_16x16x96_nse_gaps")
    setup, mesh, inp, par, sta, out = _types(g)
    setup.optimize.jobs_fun, setup.optimize.wjobs_fun = ["nse", "kge", "rmse"], [0.5, 0.3, 0.2]
    setup.optimize.wgauge = np.array([0.5, 0.3, 0.2], F32)
    smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], out, F32(0))
    s = inp._smashx_solver
    before = smash_amd.OutputDT(setup, mesh)
    s.cost_and_qsim(before)
    assert before.cost == out.cost and np.array_equal(before.qsim, out.qsim) and out.cost != 0
    rng = np.random.default_rng(3)
    other = np.asfortranarray((out.qsim * (0.5 + rng.random(out.qsim.shape))).astype(F32))
    jobs, qb, jd = s.jobs_of_qsim(other, jobs_b=1.0, qsim_d=np.asfortranarray(np.ones_like(other)))
    assert jobs != out.cost and np.any(qb) and jd != 0
    after = smash_amd.OutputDT(setup, mesh)
    s.cost_and_qsim(after)
    assert ce.same_bits(after.cost, before.cost) and ce.same_bits(after.qsim, before.qsim)
    assert ce.same_bits(after.cost_jobs, before.cost_jobs)


def test_fewer_criteria_do_not_see_the_coefficients_of_the_call_before():
    """eight criteria, then rmse alone on the same plan and series: the bits of the restatement, which the CPU test pins to the
    reference"""
    r = FIX["njf8_nolog"]
    plan = _plan(r, r["qobs"].shape[1])
    first = _probe(r, plan=plan)
    assert ce.same_bits(first[0], r["jobs"])
    second = _probe(r, jobs_fun=("rmse",), wjobs=(1.0,), plan=plan)
    c = dict(ce.cases()["njf8_nolog"], jobs=("rmse",), wjobs=np.ones(1, F32))
    for jb, got in zip(ce.JOBS_B, second[2:]):
        t = ce.restate(c, jobs_b=jb)
        assert ce.same_bits(got, t["qsim_b"]) and np.any(got)
    t = ce.restate(c)
    assert ce.same_bits(second[0], t["jobs"]) and ce.same_bits(second[1], t["jobs_d"])


# ---- gauges without data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_gauge_counts_as_weight_zero_in_jobs_of_qsim(name):
    c, gs = EMPTY[name]
    r = dict(c, jobs_fun=c["jobs"])
    w = _probe(r)
    z = _probe(r, wgauge=ce.zeroed(c, gs)["wgauge"])
    print(f"{name}: weighted jobs {w[0]!r} jobs_d {w[1]!r}; with the weight at 0 {z[0]!r} {z[1]!r}")
    bad = [k for k, a, b in zip(("jobs", "jobs_d", "qsim_b1", "qsim_b2"), w, z) if not ce.same_bits(a, b)]
    assert not bad, bad
    assert not w[2][list(gs)].any() and not w[3][list(gs)].any()
    if len(gs) < c["ng"]:
        assert np.isfinite(w[0]) and w[0] != 0 and w[1] != 0 and np.any(w[2])
        t = ce.restate(c)                      # and it is the cost of the gauges that have data (a loose bar: logf differs by build)
        assert abs(float(w[0]) - float(t["jobs"])) <= 1e-5 * abs(float(t["jobs"]))
    else:
        assert w[0] == 0 and w[1] == 0 and not np.any(w[2])


def _sweeps(g):
    return dict(_forward(g), **_adjoint(g), **{k: v for k, v in _tangent(g).items() if k != "tan.terms"})


@pytest.mark.parametrize("name", list(ce.SWEEP_EMPTY))
def test_empty_gauge_counts_as_weight_zero_in_the_sweeps(name):
    gw, gz = ce.sweep_case(name), ce.sweep_case(name, zero=True)
    w, z = _sweeps(gw), _sweeps(gz)
    bad = [k for k in w if not ce.same_bits(w[k], z[k])]
    print(f"{name}: cost {w['cost']!r} cost_d {w['cost_d']!r}; with the weight at 0 {z['cost']!r} {z['cost_d']!r}")
    assert not bad, bad
    # and both are the oracle's, by the rule of the at-size tests
    ref = {f64: jc.oracle_outputs(gw, fp64=f64) for f64 in (False, True)}
    used = gu.STRUCT_PARAMS[jc.STRUCTURE] + gu.STRUCT_STATES[jc.STRUCTURE]
    sweep = {k: w[k] for k in ("qsim", "cost", "adj.cost", "qsim_d", "cost_d")}
    sweep.update({k + "_b": w[k + "_b"] for k in used})
    assert not _check(gw.id, sweep, ref)


def _cance(weights, blank):
    g = gu.load("gr_a_cance_28x28x1440")
    q = np.array(g.qobs, F32, order="F")
    q[blank, :] = ce.MISSING
    opts = dict(g.opts, wgauge=np.array(weights, F32), jobs_fun=("nse", "kge"), wjobs_fun=(0.6, 0.4))
    return types.SimpleNamespace(**dict(vars(g), qobs=q, opts=opts))


@pytest.mark.parametrize("weights", [(0.5, 0.3, 0.2), (-1.0, -1.0, -1.0), (0.5, -1.0, -1.0)])
def test_empty_gauge_counts_as_weight_zero_in_multiple_run_and_uniform_costs(weights):
    """tests/golden/multiple_run/gr_a_cance_s16's first four samples with the second gauge's observations blanked"""
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "multiple_run", "gr_a_cance_s16.npz"))
    sample = np.asfortranarray(z["sample"][:, :4])
    zero = list(weights)
    zero[1] = 0.0
    res = {}
    for tag, w in (("weighted", weights), ("zero", zero)):
        g = _cance(w, 1)
        setup, mesh, inp, par, sta, out = _types(g)
        ec = np.zeros(4, F32)
        smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, z["ind"], ec, np.zeros(0, F32))
        uc = smash_amd.uniform_costs(setup, mesh, inp, par, sta, sample, z["ind"])
        res[tag] = (ec, np.asarray(uc, F32))
    print(weights, "multiple_run", res["weighted"][0], res["zero"][0], "uniform_costs", res["weighted"][1], res["zero"][1])
    assert ce.same_bits(res["weighted"][0], res["zero"][0]) and ce.same_bits(res["weighted"][1], res["zero"][1])
    assert np.all(np.isfinite(res["weighted"][0])) and np.all(res["weighted"][0] != 0)


def test_empty_gauge_with_a_median_slot_is_refused_and_one_observation_brings_it_back():
    import smash_amd
    from smash_amd import _lib
    from smash_amd.solver import Solver
    c, gs = EMPTY["empty_median_middle"]
    (g,) = gs
    r = dict(c, jobs_fun=c["jobs"])
    setup, _ = _plan(r, c["nt"])
    o = setup.optimize
    o.jobs_fun, o.wjobs_fun = ["se", "rmse"], [0.6, 0.4]            # (finite on a single observation: no NaN in the median)
    o.optimize_start_step, o.wgauge = int(c["start"]), np.asarray(c["wgauge"], F32)
    m = ce.base_mesh()
    mesh = smash_amd.MeshDT(setup, m.nrow, m.ncol, c["ng"])
    mesh.dx = ce.DX
    mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.flwdir, m.flwacc, m.path, m.active_cell
    mesh.gauge_pos, mesh.area = np.asfortranarray(c["gauge_pos"].astype(np.int32)), np.ascontiguousarray(c["area"], F32)
    good = c["qobs"].copy(order="F")
    good[g, c["nt"] - 1] = good[(g + 1) % c["ng"], c["nt"] - 1]                 # one observation, on the last step
    for order in ("options_then_qobs", "qobs_then_options"):
        s = Solver(setup, mesh)
        s.set_median_slots(c["ng"], np.arange(c["ng"], dtype=np.int32), reduce_fn=lambda a: None)
        with pytest.raises(smash_amd.SmashxError) as e:
            if order == "options_then_qobs":
                s.set_options(o)                     # (no observations yet: nothing to refuse)
                s.set_qobs(c["qobs"])
            else:
                s.set_qobs(c["qobs"])                # (the plan's default weights are positive: nothing to refuse)
                s.set_options(o)
        assert e.value.code == _lib.E_UNSUPPORTED, e.value
        s.set_qobs(good)
        s.set_options(o)
        jobs, qb, jd = s.jobs_of_qsim(c["qsim"], jobs_b=1.0, qsim_d=c["qsim_d"])
        want = ce.restate(dict(c, qobs=good, jobs=("se", "rmse"), wjobs=np.array([0.6, 0.4], F32)))
        print(order, "jobs", jobs, float(want["jobs"]), "jobs_d", jd, float(want["jobs_d"]))
        # (the slot path forms the median as a weighted sum of the two points: not the reference's expression, a rounding or two away)
        assert abs(float(jobs) - float(want["jobs"])) <= 1e-6 * abs(float(want["jobs"])) and np.any(qb)            # (a median of four again)
        with pytest.raises(smash_amd.SmashxError) as e:          # ... and blanking it again is refused again, by set_qobs
            s.set_qobs(c["qobs"])
        assert e.value.code == _lib.E_UNSUPPORTED
        s.close()
    # the slots declared last, on a plan that already dropped the gauge: refused by that call
    s = Solver(setup, mesh)
    s.set_qobs(c["qobs"])
    s.set_options(o)
    with pytest.raises(smash_amd.SmashxError) as e:
        s.set_median_slots(c["ng"], np.arange(c["ng"], dtype=np.int32), reduce_fn=lambda a: None)
    assert e.value.code == _lib.E_UNSUPPORTED
    s.close()


# ---- two gauges on one cell ----------------------------------------------------------------------------------------------------------------
def test_two_gauges_on_one_cell_vs_oracle():
    g = ce.shared_cell_case()
    hip = _sweeps(g)
    ref = {f64: jc.oracle_outputs(g, fp64=f64) for f64 in (False, True)}
    used = gu.STRUCT_PARAMS[jc.STRUCTURE] + gu.STRUCT_STATES[jc.STRUCTURE]
    sweep = {k: hip[k] for k in ("qsim", "cost", "adj.cost", "qsim_d", "cost_d")}
    sweep.update({k + "_b": hip[k + "_b"] for k in used})
    assert np.array_equal(hip["qsim"][0], hip["qsim"][1]) and any(np.any(hip[k + "_b"]) for k in used)
    # both gauges seed the cell: with the second gauge's weight at 0 the gradient is another one
    g0 = ce.shared_cell_case()
    g0.opts["wgauge"] = np.array([0.6, 0.0], F32)
    assert not ce.same_bits(_adjoint(g0)["cp_b"], hip["cp_b"])
    assert not _check(g.id, sweep, ref)


N_TESTS = len(FIX) + 2 + len(EMPTY) + len(ce.SWEEP_EMPTY) + 3 + 1 + 1


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
