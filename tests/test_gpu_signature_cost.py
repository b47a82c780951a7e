"""GPU: the signature-based criteria Crc, Cfp2/10/50/90, Epf, Elt, Erc in the cost of the forward, adjoint and tangent sweeps, against
what the compiled reference computed (tests/golden/signature_cost/, recorded by tests/golden/make_signature_cost.py).

Function level.  The cost kernels are fed the hand-made series through smashx_jobs_of_qsim (include/smashx_signature.h), which runs
compute_jobs / _B / _D on a prescribed discharge: a plan with ONE gauge on a headwater cell (flwacc = 1), area = 1 m2, dt = 1 s,
dx = 1 m, so that the kernels' qo = qobs x 1000 and qs = qsim x 1000 exactly as the recorder formed them from the stored raw series.
The series sits behind five steps of junk that optimize_start_step = 6 cuts off.  The criteria hold no libm call: cost, qsim_b and the
tangent must equal the reference's BIT FOR BIT in both builds of the library.

End to end.  forward / forward_b / forward_d through the Python drop-in on two golden inputs with eight criteria at once, and with the
median over gauges and a late start step.  Under the exact-libm build (the last test runs this module again with SMASHX_EXACT_LIBM=1)
the discharge, the cost and every gradient field must equal the reference's bit for bit (the tangent: see _check_against_fixture); the
default build is held to the bars tests/test_gpu_parity.py uses for it (golden_util.tol: 1e-6, relaxed per output to 3 x the reference's
own flag-to-flag noise on that output), with the noise the recorder measured on THESE outputs between the reference's -O3 + FMA build
and its parity build.  It is large here -- up to 1.5e-2 on a gradient field of the Cance case with eight criteria -- because the
percentiles and the event maxima select time steps: a last-bit difference in the discharge moves a seed to another step.  Measured on
an MI355X, default build against the fixtures: cost within 4e-7 relative (6e-6 with the median, where the reference's builds differ by
1.1e-5), gradient fields within 2.1e-4 where the reference's two builds differ by 1.4e-3 ... 1.5e-2, within 2.3e-5 elsewhere;
exact-libm build: discharge, cost and every gradient field bit-identical; qsim_d off in the last bit on a few steps."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import signature_util as su
from smash_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FUN = su.load_functions()
PAD = 5
K = np.float32(1e3)


def _exact():
    from smash_amd import _lib
    return _lib.EXACT


# ---- function level --------------------------------------------------------------------------------------------------------------------
def _one_gauge_plan(nt):
    """a plan over the 12 x 12 mesh of a golden fixture with a single gauge on a headwater cell, unit area, dt = dx = 1"""
    import smash_amd
    from smash_amd.solver import Solver
    g = gu.load("gr_a_12x12x48_nse")
    m = g.mesh
    r, c = [int(v[0]) for v in np.nonzero((np.asarray(m.flwacc) == 1) & (np.asarray(m.active_cell) == 1))]
    setup = smash_amd.SetupDT(0, 1, structure="gr-a", dt=1.0, ntime_step=nt)
    mesh = smash_amd.MeshDT(setup, m.nrow, m.ncol, 1)
    mesh.dx = 1.0
    mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.flwdir, m.flwacc, m.path, m.active_cell
    mesh.gauge_pos = np.asfortranarray(np.array([[r, c]], np.int32))
    mesh.area = np.ones(1, np.float32)
    return setup, Solver(setup, mesh)


def _padded(a, fill, dtype):
    out = np.full((1, PAD + a.size), fill, dtype, order="F")
    out[0, PAD:] = a
    return out


def test_percentile_sort_in_the_plans_scratch(monkeypatch):
    """SMASHX_SIG_LDS=0 sends the percentiles' sort to the plan's scratch buffers, the path a series too long for the LDS takes: the
    same bits as the LDS path on the tie case and on the case that recompacts the observed series"""
    monkeypatch.setenv("SMASHX_SIG_LDS", "0")
    for case in ("tie_zeros", "compact2", "len129"):
        test_function_level_fixtures_through_the_c_abi(case)


def test_replayed_sort_and_selection_give_the_same_bits(monkeypatch):
    """SMASHX_SIG_REPLAY=1 forces the reference's heap sort where the default path selects the two interpolation points without
    sorting (taken when each occurs once; the tie case replays either way): every function-level series and the eight-criterion
    fixtures on the reference's discharge must come out bit for bit as they do by default, i.e. as the reference has them"""
    monkeypatch.setenv("SMASHX_SIG_REPLAY", "1")
    for case in sorted(FUN):
        test_function_level_fixtures_through_the_c_abi(case)
    for case in su.E2E_CASES:
        test_cost_kernels_on_the_reference_discharge(case, "all")


@pytest.mark.parametrize("case", sorted(FUN))
def test_function_level_fixtures_through_the_c_abi(case):
    c = FUN[case]
    n = c["qo"].size
    setup, s = _one_gauge_plan(PAD + n)
    z = np.load(os.path.join(su.DIR, "functions.npz"))
    raw = {k: z[f"{case}__raw_{k}"] for k in ("qobs", "qsim", "qsim_d")}
    assert su.same_bits(raw["qobs"] * K, c["qo"]) and su.same_bits(raw["qsim"] * K, c["qs"]) and su.same_bits(raw["qsim_d"] * K, c["qs_d"])
    qobs = _padded(raw["qobs"], 0.004, np.float32)
    qsim = _padded(raw["qsim"], 0.007, np.float32)
    qsim_d = _padded(raw["qsim_d"], 0.5, np.float32)
    po = _padded(c["po"], 9.0, np.float32)
    mask = _padded(c["mask"], 0, np.int32)
    mask[0, 1:4] = max(int(c["mask"].max()), 1)          # junk in front of the start step: an event number that also occurs later
    s.set_qobs(qobs)
    s.set_signature_inputs(po, mask)
    o = setup.optimize
    o.optimize_start_step, o.wgauge = PAD + 1, np.ones(1, np.float32)
    bad = {}
    for nm, (res, qs_b, res_d) in c["crit"].items():
        o.jobs_fun, o.wjobs_fun = [nm], [1.0]
        s.set_options(o)
        jobs, qsim_b, jobs_d = s.jobs_of_qsim(qsim, jobs_b=1.0, qsim_d=qsim_d)
        want_b = np.float32(0) + np.float32(1e3) * qs_b / np.float32(1)            # forward_db.f90:2709-2712 with dt = area = 1
        print(f"{case} {nm}: jobs {jobs!r} (reference {res!r}), jobs_d {jobs_d!r} ({res_d!r}), seeds on {np.flatnonzero(qsim_b[0]).tolist()[:6]}")
        if not (su.same_bits(jobs, res) and su.same_bits(jobs_d, res_d) and su.same_bits(qsim_b[0, PAD:], want_b) and not qsim_b[0, :PAD].any()):
            bad[nm] = (jobs, res, jobs_d, res_d, np.flatnonzero(qsim_b[0, PAD:] != want_b).tolist()[:8])
    assert not bad, bad
    s.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _setup(case, tag, residency="dense", mean_prcp=None):
    """the types of a golden input with the criteria, weights, start step and mask of fixture <case>__<tag>"""
    import smash_amd
    from test_gpu_parity import _types
    g = gu.load(case)
    z = su.load_e2e(case, tag)
    kw = {}
    if residency == "compact":
        from test_gpu_compact import SYNTH_LAYOUT
        kw["layout"] = dict(SYNTH_LAYOUT) if "cance" not in case else dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1)
    setup, mesh, inp, par, sta, out = _types(g, **kw)
    o = setup.optimize
    o.jobs_fun, o.wjobs_fun = [str(j) for j in z["jobs_fun"]], [float(w) for w in z["wjobs_fun"]]
    o.wgauge, o.optimize_start_step = np.asarray(z["wgauge"], np.float32), int(z["optimize_start_step"])
    o.mask_event = np.asfortranarray(z["mask_event"])
    if mean_prcp is None:
        mean_prcp = np.load(os.path.join(gu.GOLDEN_DIR, "mean_forcing", case + ".npz"))["mean_prcp"]
    inp.mean_prcp = np.asfortranarray(mean_prcp)
    if residency == "sparse":
        setup.sparse_storage = True
        act = g.mesh.active_cell
        idx = [(r, c) for r, c in zip(g.mesh.path[0], g.mesh.path[1]) if r >= 0 and c >= 0 and act[r, c] == 1]
        rr, cc = np.array([i[0] for i in idx]), np.array([i[1] for i in idx])
        inp2 = smash_amd.Input_DataDT(setup, mesh)
        inp2.sparse_prcp, inp2.sparse_pet = np.asfortranarray(g.prcp[rr, cc, :]), np.asfortranarray(g.pet[rr, cc, :])
        inp2.qobs, inp2.mean_prcp, inp2._bgd = g.qobs, inp.mean_prcp, inp._bgd
        inp = inp2
    return g, z, setup, mesh, inp, par, sta, out


def _sweeps(g, z, setup, mesh, inp, par, sta, out):
    """forward, forward_b and forward_d through the Python drop-in: (cost, qsim, gradients, cost_d, qsim_d)"""
    import smash_amd
    cost = smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    qsim = out.qsim.copy()
    par_b, sta_b = par.copy(), sta.copy()
    cost_b = smash_amd.forward_b(setup, mesh, inp, par.copy(), par_b, inp._bgd[0], par.copy(), sta.copy(), sta_b, inp._bgd[1], sta.copy(),
                                 out, out.copy(), np.float32(0), np.float32(1))
    assert cost_b == cost and np.array_equal(out.qsim, qsim)
    par_d = smash_amd.ParametersDT.from_dict(mesh, {k: z["d_" + k] for k in gu.STRUCT_PARAMS[g.structure]})
    sta_d = smash_amd.StatesDT.from_dict(mesh, {k: z["d_" + k] for k in gu.STRUCT_STATES[g.structure]})
    for k in synth.PARAM_NAMES:
        if k not in gu.STRUCT_PARAMS[g.structure]:
            getattr(par_d, k)[...] = 0.0
    for k in synth.STATE_NAMES:
        if k not in gu.STRUCT_STATES[g.structure]:
            getattr(sta_d, k)[...] = 0.0
    out_d = smash_amd.OutputDT(setup, mesh)
    _, cost_d = smash_amd.forward_d(setup, mesh, inp, par.copy(), par_d, inp._bgd[0], par.copy(), sta.copy(), sta_d, inp._bgd[1], sta.copy(),
                                    out, out_d)
    grads = {k: np.array(getattr(par_b, k)) for k in gu.STRUCT_PARAMS[g.structure]}
    grads.update({k: np.array(getattr(sta_b, k)) for k in gu.STRUCT_STATES[g.structure]})
    return np.float32(cost), qsim, grads, np.float32(cost_d), out_d.qsim.copy()


def _check_against_fixture(g, z, res, where):
    cost, qsim, grads, cost_d, qsim_d = res
    fig = {"cost": (float(cost), float(z["cost"])), "cost_d": (float(cost_d), float(z["cost_d"])),
           "qsim": max(gu.rel_l2(qsim[i], z["qsim"][i]) for i in range(qsim.shape[0])),
           "qsim_d": max(gu.rel_l2(qsim_d[i], z["qsim_d"][i]) for i in range(qsim.shape[0]))}
    fig.update({k + "_b": gu.rel_l2(v, z["b_" + k]) for k, v in grads.items()})
    print(where, "exact-libm" if _exact() else "default", fig)
    if _exact():
        # bit equality of the discharge, the cost and every gradient field
        assert su.same_bits(qsim, z["qsim"]) and su.same_bits(cost, z["cost"]), fig
        differ = {k: int(np.count_nonzero(v != z["b_" + k])) for k, v in grads.items() if not np.array_equal(v, z["b_" + k])}
        assert not differ, (differ, fig)
        # The tangent is not bit-identical in this build either, and not because of these criteria: the reference's forward_d
        # (Tapenade's tangent code of the operators, forward_db.f90) evaluates the primal and its derivative in re-associated
        # expressions, the library's tangent kernels (sx_tangent.h) in the operators' own order; qsim_d differs in the last bit on a
        # few steps whatever the cost is.  tests/test_gpu_tangent.py bars it at
        # 1e-6 (qsim_d) and 1e-5 (cost_d); the same here, WITHOUT the relaxation by the reference's noise.
        for i in range(qsim.shape[0]):
            assert gu.rel_l2(qsim_d[i], z["qsim_d"][i]) <= 1e-6, fig
        assert abs(cost_d - z["cost_d"]) <= 1e-5 * abs(float(z["cost_d"])), fig
        return
    else:
        for i in range(qsim.shape[0]):
            assert gu.rel_l2(qsim[i], z["qsim"][i]) <= gu.tol(z["noise_qsim"][i]), fig
        assert abs(cost - z["cost"]) <= gu.tol_cost(float(z["noise_cost"]), float(z["cost"])), fig
        for k, v in grads.items():
            assert gu.rel_l2(v, z["b_" + k]) <= gu.tol(float(z["noise_b_" + k])), (k, fig, float(z["noise_b_" + k]))
    # the tangent as tests/test_gpu_tangent.py bars it: 1e-6 on qsim_d and 1e-5 on cost_d (its primal is forward_d's re-associated
    # one), each relaxed to 3 x the reference's own noise
    for i in range(qsim.shape[0]):
        assert gu.rel_l2(qsim_d[i], z["qsim_d"][i]) <= gu.tol(z["noise_qsim_d"][i]), fig
    assert abs(cost_d - z["cost_d"]) <= gu.tol(float(z["noise_cost_d"]), base=1e-5) * abs(float(z["cost_d"])), fig


@pytest.mark.parametrize("tag", ["all", "median"])
@pytest.mark.parametrize("case", su.E2E_CASES)
def test_end_to_end_sweeps_and_forcing_residencies(case, tag):
    """cost, every gradient field and the tangent of the three sweeps against the reference; then the sparse and the compact residency
    of the forcing against the dense one, bit for bit"""
    g, z, *types = _setup(case, tag)
    dense = _sweeps(g, z, *types)
    _check_against_fixture(g, z, dense, f"{case} {tag}")
    for residency in ("sparse", "compact"):
        g2, z2, *types2 = _setup(case, tag, residency)
        if residency == "compact" and "cance" not in case:
            assert types2[2]._smashx_solver.forcing_info()["layout"].startswith("compact")
        other = _sweeps(g2, z2, *types2)
        assert su.same_bits(other[0], dense[0]) and su.same_bits(other[3], dense[3]), residency
        assert np.array_equal(other[1], dense[1]) and np.array_equal(other[4], dense[4]), residency
        for k in dense[2]:
            assert np.array_equal(other[2][k], dense[2][k]), (residency, k)


@pytest.mark.parametrize("tag", ["all", "median"])
@pytest.mark.parametrize("case", su.E2E_CASES)
def test_cost_kernels_on_the_reference_discharge(case, tag):
    """The cost kernels alone on the discharge the reference itself simulated (smashx_jobs_of_qsim): cost and qsim_b must equal the
    reference's bit for bit in BOTH builds -- nse, kge and the signatures hold no libm call.  The tangent of the cost along the
    reference's qsim_d is barred like cost_d in tests/test_gpu_tangent.py (1e-5): the reference forms it on forward_d's own primal."""
    g, z, setup, mesh, inp, par, sta, out = _setup(case, tag)
    from smash_amd.solver import _solver_for
    s = _solver_for(setup, mesh, inp)
    jobs, qsim_b, jobs_d = s.jobs_of_qsim(np.asfortranarray(z["qsim"]), jobs_b=1.0, qsim_d=np.asfortranarray(z["qsim_d"]))
    print(case, tag, "jobs", jobs, float(z["cost"]), "jobs_d", jobs_d, float(z["cost_d"]), "qsim_b differs on",
          int(np.count_nonzero(qsim_b != z["qsim_b"])), "of", int(np.count_nonzero(z["qsim_b"])), "seeded entries")
    assert su.same_bits(jobs, z["cost"])
    assert su.same_bits(qsim_b, np.asfortranarray(z["qsim_b"]))
    assert abs(jobs_d - z["cost_d"]) <= 1e-5 * abs(float(z["cost_d"]))


def test_mean_forcing_output_feeds_the_criteria_and_a_mask_changed_in_place_is_seen():
    """smash_amd.compute_mean_forcing writes input_data.mean_prcp on the GPU; the criteria read it as it is (the same bits as the
    recorded one, tests/test_gpu_mean_forcing.py).  Then mask_event is edited IN PLACE: the next call must see it."""
    import smash_amd
    case = "gr_a_cance_28x28x1440"
    g, z, setup, mesh, inp, par, sta, out = _setup(case, "all")
    recorded = inp.mean_prcp.copy()
    inp.mean_prcp = np.full(recorded.shape, -99.0, np.float32, order="F")
    smash_amd.compute_mean_forcing(setup, mesh, inp)
    assert su.same_bits(inp.mean_prcp, recorded)
    c1 = smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    g0, z0, *fresh = _setup(case, "all")
    c0 = smash_amd.forward(fresh[0], fresh[1], fresh[2], fresh[3].copy(), fresh[2]._bgd[0], fresh[4].copy(), fresh[2]._bgd[1], fresh[5], np.float32(0))
    assert c1 == c0
    solver = inp._smashx_solver
    mk = setup.optimize.mask_event
    first = np.flatnonzero(mk[0] == 1)
    mk[0, first[: len(first) // 2]] = 0                       # the first event of gauge 1 loses its first half
    c2 = smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    assert inp._smashx_solver is solver and c2 != c1
    fresh[0].optimize.mask_event = mk.copy(order="F")
    c3 = smash_amd.forward(fresh[0], fresh[1], fresh[2], fresh[3].copy(), fresh[2]._bgd[0], fresh[4].copy(), fresh[2]._bgd[1], fresh[5], np.float32(0))
    assert c2 == c3


def test_refusals():
    """every refusal of include/smashx_signature.h, at the C ABI (the Python host refuses the first two itself, before the device)"""
    import smash_amd
    from smash_amd import _lib
    from smash_amd.solver import Solver
    g, z, setup, mesh, inp, par, sta, out = _setup("gr_b_16x16x96_nse_gaps", "all")
    o = setup.optimize
    s = Solver(setup, mesh)
    s.set_forcing(inp.prcp, inp.pet)
    s.set_qobs(inp.qobs)

    def refused(jobs, code=_lib.E_UNSUPPORTED):
        o.jobs_fun, o.wjobs_fun = list(jobs), [1.0] * len(jobs)
        with pytest.raises(smash_amd.SmashxError) as e:
            s.set_options(o)
        assert e.value.code == code, e.value
    refused(["Crc"])                                            # before smashx_set_signature_inputs
    s.set_signature_inputs(inp.mean_prcp)
    refused(["nse", "Epf"])                                     # an E* criterion without mask_event
    o.jobs_fun, o.wjobs_fun = ["Cfp50", "Crc"], [0.5, 0.5]
    s.set_options(o)                                            # ... while the others are accepted
    s.set_signature_inputs(np.full_like(inp.mean_prcp, -99.0), o.mask_event)
    refused(["Crc"])                                            # the -99 prefill: Crc would divide by a sum it never formed
    with pytest.raises(smash_amd.SmashxError) as e:             # the refusal left no usable options: a sweep says so
        s.upload(par, sta, par, sta)
        s.sweep(False)
    assert e.value.code == _lib.E_STATE
    dry = inp.mean_prcp.copy(order="F")
    first = np.flatnonzero(o.mask_event[1] == 1)
    dry[1, first] = 0.0
    s.set_signature_inputs(dry, o.mask_event)
    refused(["Erc"])                                            # the first event of gauge 2 has no rain: nothing was assigned before it
    o.wgauge = np.array([1.0, 0.0, 0.0], np.float32)
    o.jobs_fun, o.wjobs_fun = ["Erc"], [1.0]
    s.set_options(o)                                            # ... unless that gauge is not evaluated
    s.set_signature_inputs(inp.mean_prcp, o.mask_event)
    o.jobs_fun, o.wjobs_fun = ["nse", "Crc"], [0.5, 0.5]
    s.set_options(o)
    s.upload(par, sta, par, sta)
    with pytest.raises(smash_amd.SmashxError) as e:             # the ensemble cost
        s.multiple_run(par, sta, np.asfortranarray(np.array([[100.0, 200.0]], np.float32)), np.array([2], np.int32))
    assert e.value.code == _lib.E_UNSUPPORTED
    bad = o.mask_event.copy(order="F")
    bad[0, 0] = -3
    rc = _lib.lib().smashx_set_signature_inputs(s._h, inp.mean_prcp.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p))
    assert rc == _lib.E_ARG
    assert _lib.lib().smashx_set_signature_inputs(s._h, None, None) == _lib.E_ARG
    s.close()
    # tiled plans
    t = Solver(setup, mesh, tile=(0, mesh.nrow, mesh.ncol // 2, mesh.ncol))          # (the half that holds the three gauges)
    with pytest.raises(smash_amd.SmashxError) as e:
        t.set_signature_inputs(inp.mean_prcp, o.mask_event)
    assert e.value.code == _lib.E_UNSUPPORTED
    t.close()
    # the Python host: caught before anything reaches a device
    inp.mean_prcp = np.full_like(inp.mean_prcp, -99.0)
    o.jobs_fun, o.wjobs_fun, o.wgauge = ["Crc"], [1.0], np.asarray(z["wgauge"], np.float32)
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.forward(setup, mesh, inp, par, par.copy(), sta, sta.copy(), out, np.float32(0))
    assert e.value.code == _lib.E_UNSUPPORTED


def test_the_classic_criteria_take_the_code_they_took():
    """a plan that was given signature inputs and then plain options computes what a plan without them computes"""
    import smash_amd
    from test_gpu_parity import _run_adjoint
    g, z, setup, mesh, inp, par, sta, out = _setup("gr_b_16x16x96_nse_gaps", "all")
    smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    setup.optimize.jobs_fun, setup.optimize.wjobs_fun = ["nse"], [1.0]
    setup.optimize.wgauge = np.full(3, 1.0 / 3.0, np.float32)
    par_b, sta_b = par.copy(), sta.copy()
    smash_amd.forward_b(setup, mesh, inp, par.copy(), par_b, inp._bgd[0], par.copy(), sta.copy(), sta_b, inp._bgd[1], sta.copy(), out,
                        out.copy(), np.float32(0), np.float32(1))
    ref = _run_adjoint(g)
    assert out.cost == ref[2].cost and np.array_equal(out.qsim, ref[2].qsim)
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(par_b, k), getattr(ref[3], k)), k


def test_exact_libm_build_on_the_same_fixtures():
    """this module again under the exact-libm build (the library is chosen at import time): bit equality on all fixtures"""
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-s",
                        "-k", "function_level or end_to_end or reference_discharge or scratch or replayed"], env=env, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    sys.stdout.write("\n".join(ln for ln in r.stdout.splitlines() if "exact-libm {" in ln) + "\n" + r.stdout[-3000:])
    assert r.returncode == 0 and "20 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
