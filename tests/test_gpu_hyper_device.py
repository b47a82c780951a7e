"""GPU: the hyper maps on the device (include/smashx_hyper.h, smash_amd/csrc/sx_hypermap.h) and smash_amd.optimize_hyper_lbfgsb over
them.  The oracle is the host map of the same library (smashx_hyper_map_forward / _b, sx_hyper.cpp: code these calls do not touch, pinned
to the reference by tests/test_hyper_cpu.py) or the reference's fixtures directly; every check holds in both builds (the default one
and SMASHX_EXACT_LIBM=1).  Synthetic descriptors are drawn in [0, 1] over the whole grid with exact 0 and exact 1 present -- what the
calibration's normalisation produces; with such inputs an inactive cell of the host path adds only zeros to the whole-grid sums, which
are therefore comparable bit for bit with the device's sums over the active cells."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import golden_util as gu  # noqa: E402
import hyper_device_util as hu  # noqa: E402
import make_golden as mg  # noqa: E402
from test_hyper_cpu import _case  # noqa: E402

pytestmark = pytest.mark.gpu


def _solver(setup, mesh, inp, descriptors=True):
    from smash_amd.solver import _plain, _solver_for
    s = _solver_for(_plain(setup), mesh, inp)
    if descriptors:
        s.set_hyper_descriptors(setup.optimize.mapping, np.asfortranarray(inp.descriptor, dtype=np.float32))
    return s


def _host_fields(setup, mesh, inp, HP, HS):
    import smash_amd
    from smash_amd.solver import _hyper_to_fields
    p, s = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    _hyper_to_fields(setup, mesh, inp, p, HP, s, HS)
    return p, s


def _device_fields(sol, mesh, fill=-7.0):
    import smash_amd
    from smash_amd import synth
    p, s = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    for o, names in ((p, synth.PARAM_NAMES), (s, synth.STATE_NAMES)):
        for k in names:
            getattr(o, k)[...] = fill
    sol.hyper_fields(p, s)
    return p, s


# ---- 1. the forward map against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mapping", mg.HYPER_CASES)
def test_forward_map_vs_reference_golden(name, mapping):
    from smash_amd import synth
    g, z, setup, mesh, inp, par, sta, HP, HS = _case(name, mapping)
    sol = _solver(setup, mesh, inp)
    sol.hyper_upload(HP.matrix(), HS.matrix())
    p, s = _device_fields(sol, mesh)
    act = np.asarray(mesh.active_cell) == 1
    hp, hs = _host_fields(setup, mesh, inp, HP, HS)
    for k in synth.PARAM_NAMES:
        assert hu.same_bits(getattr(p, k)[act], z["fwd_p_" + k][act]), k
        assert np.all(getattr(p, k)[~act] == -7.0), k                 # the rest is left as the caller had it
    for k in synth.STATE_NAMES:
        assert hu.same_bits(getattr(s, k)[act], getattr(hs, k)[act]), k
        assert np.all(getattr(s, k)[~act] == -7.0), k


# ---- 2. / 3. a masked D8 mesh whose cell count is no multiple of 64 ----------------------------------------------------------------------------
SYNTH = [("gr-b", "hyper-linear", 1), ("gr-b", "hyper-polynomial", 6), ("gr-b", "hyper-linear", 0), ("gr-b", "hyper-polynomial", 0),
         ("vic-a", "hyper-linear", 1), ("vic-a", "hyper-polynomial", 6), ("vic-a", "hyper-linear", 0)]


def _synth_case(structure, mapping, nd, nt=24):
    import smash_amd
    from smash_amd import synth
    from smash_amd.types import GLB_PARAMETERS, GLB_STATES, GUB_PARAMETERS, GUB_STATES
    m = synth.make_mesh_d8(33, 29, ng=3, radius=0.45)
    assert m.nac % 64 != 0 and 256 < m.nac < 33 * 29
    rng = np.random.default_rng(1000 * nd + len(structure) + len(mapping))
    prcp, pet = synth.dense_forcing(m, nt)
    setup = smash_amd.SetupDT(nd, m.ng, structure=structure, dt=3600.0, ntime_step=nt)
    o = setup.optimize
    o.mapping, o.nhyper = mapping, 1 + nd * (2 if mapping == "hyper-polynomial" else 1)
    o.jobs_fun, o.wjobs_fun = ["nse"], [1.0]
    mesh = smash_amd.MeshDT.from_synth(setup, m)
    inp = smash_amd.Input_DataDT(setup, mesh)
    inp.prcp, inp.pet = prcp, pet
    inp.qobs = np.asfortranarray((0.2 + 3.0 * rng.random((m.ng, nt))).astype(np.float32))
    desc = np.asfortranarray(rng.random((33, 29, nd)).astype(np.float32))
    rr, cc = np.nonzero(np.asarray(m.active_cell) == 1)
    for j in range(nd):                       # exact 0 and exact 1, on active cells and outside them
        desc[rr[3 + j], cc[3 + j], j], desc[rr[-5 - j], cc[-5 - j], j] = 0.0, 1.0
        desc[0, j, j], desc[32, 28 - j, j] = 0.0, 1.0
    inp.descriptor = desc
    # intercepts at the logit of ordinary field values, coefficients of either sign, exponents of exactly 1 and others in [0.5, 2]
    P, S = synth.make_parameters(33, 29), synth.make_states(33, 29, warm=True)

    def mat(vals, names, lb, ub):
        H = np.zeros((o.nhyper, len(names)), np.float32, order="F")
        for i, k in enumerate(names):
            t = min(max((float(np.mean(vals[k])) - lb[i]) / (ub[i] - lb[i]), 1e-3), 1 - 1e-3)
            H[0, i] = np.log(t / (1 - t))
            if mapping == "hyper-linear":
                H[1:, i] = 0.3 * rng.standard_normal(nd)
            else:
                H[1::2, i] = 0.3 * rng.standard_normal(nd)
                e = (0.5 + 1.5 * rng.random(nd)).astype(np.float32)
                e[(np.arange(nd) + i) % 3 == 0] = 1.0
                H[2::2, i] = e
        return H
    return setup, mesh, inp, mat(P, synth.PARAM_NAMES, GLB_PARAMETERS, GUB_PARAMETERS), mat(S, synth.STATE_NAMES, GLB_STATES, GUB_STATES)


def _hyper_objects(setup, hpm, hsm):
    import smash_amd
    HP, HS = smash_amd.Hyper_ParametersDT(setup), smash_amd.Hyper_StatesDT(setup)
    HP.set_matrix(hpm)
    HS.set_matrix(hsm)
    return HP, HS


@pytest.mark.parametrize("structure,mapping,nd", SYNTH)
def test_forward_map_across_block_edges(structure, mapping, nd):
    from smash_amd import synth
    setup, mesh, inp, hpm, hsm = _synth_case(structure, mapping, nd)
    if mapping == "hyper-polynomial" and nd:
        assert np.any(hpm[2::2] == 1.0) and np.any(hpm[2::2] != 1.0)
    sol = _solver(setup, mesh, inp)
    sol.hyper_upload(hpm, hsm)
    p, s = _device_fields(sol, mesh)
    hp, hs = _host_fields(setup, mesh, inp, *_hyper_objects(setup, hpm, hsm))
    act = np.asarray(mesh.active_cell) == 1
    for o, h, names in ((p, hp, synth.PARAM_NAMES), (s, hs, synth.STATE_NAMES)):
        for k in names:
            assert hu.same_bits(getattr(o, k)[act], getattr(h, k)[act]), k
            assert np.all(getattr(o, k)[~act] == -7.0), k
            if nd == 0:
                assert np.unique(getattr(o, k)[act]).size == 1, k           # a constant per field


def _device_gradient(sol, setup, mesh, inp, hpm, hsm, span=None):
    """hyper_upload -> adjoint sweep -> hyper_gradient; also the gradient planes of the sweep"""
    import smash_amd
    out = smash_amd.OutputDT(setup, mesh)
    sol.hyper_upload(hpm, hsm)
    sol.sweep(True, 1.0)
    par_b, sta_b = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    cost = sol.download(True, None, None, out, par_b, sta_b)
    hpb, hsb = _gradient_with_span(sol, span)
    return cost, out, par_b, sta_b, hpb, hsb


def _gradient_with_span(sol, span=None):
    """hyper_gradient of the sweep the plan holds, with the default span or SMASHX_HYPER_SPAN = span"""
    old = os.environ.pop("SMASHX_HYPER_SPAN", None)
    try:
        if span is not None:
            os.environ["SMASHX_HYPER_SPAN"] = str(span)
        return sol.hyper_gradient()
    finally:
        os.environ.pop("SMASHX_HYPER_SPAN", None)
        if old is not None:
            os.environ["SMASHX_HYPER_SPAN"] = old


def _unread_columns_are_zero(structure, hpb, hsb):
    from smash_amd import synth
    for names, used, M in ((synth.PARAM_NAMES, gu.STRUCT_PARAMS[structure], hpb), (synth.STATE_NAMES, gu.STRUCT_STATES[structure], hsb)):
        for i, k in enumerate(names):
            if k in used:
                assert np.any(M[:, i] != 0), k
            else:
                assert hu.same_bits(M[:, i], np.zeros(M.shape[0], np.float32)), k


@pytest.mark.parametrize("structure,mapping,nd", SYNTH)
def test_adjoint_map_equals_the_host_map(structure, mapping, nd):
    setup, mesh, inp, hpm, hsm = _synth_case(structure, mapping, nd)
    sol = _solver(setup, mesh, inp)
    cost, out, par_b, sta_b, hpb, hsb = _device_gradient(sol, setup, mesh, inp, hpm, hsm)
    assert np.isfinite(cost) and np.all(np.isfinite(hpb)) and np.all(np.isfinite(hsb))
    ref_p, ref_s = hu.host_map_b(setup, mesh, inp, hpm, hsm, par_b.as_dict(), sta_b.as_dict())
    assert hu.same_bits(hpb, ref_p) and hu.same_bits(hsb, ref_s)
    _unread_columns_are_zero(structure, hpb, hsb)
    info = sol.hyper_info()
    nslot = len(gu.STRUCT_PARAMS[structure]) + len(gu.STRUCT_STATES[structure])
    assert info["chains"] == nslot * setup.optimize.nhyper and info["span"] == sol.ncells      # the default span holds this mesh whole
    if nd == 6 and mapping == "hyper-polynomial":
        assert info["chains"] > 64                                                              # more than one wavefront of chains
    # the span forced short: at least three spans, the chains carried from one to the next -- the same bits
    short = sol.ncells // 3 - 7
    hpb2, hsb2 = _gradient_with_span(sol, short)
    assert sol.hyper_info()["span"] == short and -(-sol.ncells // short) >= 3
    assert hu.same_bits(hpb2, hpb) and hu.same_bits(hsb2, hsb)


@pytest.mark.parametrize("name,mapping", mg.HYPER_CASES)
def test_adjoint_map_vs_reference_golden(name, mapping):
    """against the fixtures' adj_hp_b_* / adj_hs_b_*, the bar tests/test_gpu_hyper.py applies: gu.tol(noise, base=5e-6)"""
    g, z, setup, mesh, inp, par, sta, HP, HS = _case(name, mapping)
    sol = _solver(setup, mesh, inp)
    cost, out, par_b, sta_b, hpb, hsb = _device_gradient(sol, setup, mesh, inp, HP.matrix(), HS.matrix())
    from smash_amd import synth
    for k in gu.STRUCT_PARAMS[g.structure]:
        i = synth.PARAM_NAMES.index(k)
        assert gu.rel_l2(hpb[:, i], z["adj_hp_b_" + k]) <= gu.tol(float(z["noise_hp_b_" + k]), base=5e-6), k
    for k in gu.STRUCT_STATES[g.structure]:
        i = synth.STATE_NAMES.index(k)
        assert gu.rel_l2(hsb[:, i], z["adj_hs_b_" + k]) <= gu.tol(float(z["noise_hs_b_" + k]), base=5e-6), k
    _unread_columns_are_zero(g.structure, hpb, hsb)


# ---- 4. one evaluation equals the composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mapping", mg.HYPER_CASES)
def test_one_evaluation_equals_the_host_composition(name, mapping):
    import smash_amd
    g, z, setup, mesh, inp, par, sta, HP, HS = _case(name, mapping)
    out_h = smash_amd.OutputDT(setup, mesh)
    HPb, HSb = HP.copy(), HS.copy()
    cost_h = smash_amd.hyper_forward_b(setup, mesh, inp, par, par.copy(), HP, HPb, HP.copy(), sta, sta.copy(), HS, HSb, HS.copy(), out_h,
                                       out_h.copy(), np.float32(0), np.float32(1))
    sol = _solver(setup, mesh, inp)
    cost_d, out_d, par_b, sta_b, hpb, hsb = _device_gradient(sol, setup, mesh, inp, HP.matrix(), HS.matrix())
    assert hu.same_bits(np.float32(cost_d), np.float32(cost_h))
    assert hu.same_bits(out_d.qsim, out_h.qsim)
    assert hu.same_bits(hpb, HPb.matrix()) and hu.same_bits(hsb, HSb.matrix())


# ---- 5. calibration ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", hu.MAPPINGS)
def test_calibration_on_the_device_equals_the_host_path_and_follows_the_reference(mapping):
    import smash_amd
    res = {}
    for device_map in (True, False):
        for it in (1, 4):
            g, z, setup, mesh, inp, par, sta, out = hu.calibration_case(mapping, it)
            before = inp.descriptor.copy(order="F")
            h = smash_amd.optimize_hyper_lbfgsb(setup, mesh, inp, par, sta, out, device_map=device_map)
            res[device_map, it] = (h, par, out)
            assert hu.same_bits(inp.descriptor, before)                          # the descriptors are the caller's again
            o = setup.optimize
            assert par.cp.std() > 0 and np.all(par.cp > max(1.0, o.lb_parameters[1])) and np.all(par.cp < o.ub_parameters[1])   # denormalised, whole grid
            assert abs(float(out.cost) - h["final_cost"]) == 0
    for it in (1, 4):
        (hd, pd, od), (hh, ph, oh) = res[True, it], res[False, it]
        print(mapping, it, "device", hd["cost"], hd["final_cost"], "host", hh["cost"], hh["final_cost"])
        assert hd["cost"] == hh["cost"] and hd["final_cost"] == hh["final_cost"] and hd["cost_initial"] == hh["cost_initial"]
        assert hd["nfg"] == hh["nfg"]
        assert hu.same_bits(hd["hyper_parameters"], hh["hyper_parameters"]) and hu.same_bits(hd["hyper_states"], hh["hyper_states"])
        assert hu.same_bits(pd.cp, ph.cp) and hu.same_bits(od.qsim, oh.qsim)
    ref = {int(m): float(z[f"cost_{int(m)}"]) for m in z["maxiters"]}
    one, four = res[True, 1][0], res[True, 4][0]
    print(mapping, "reference", ref, list(z["iter_costs_4"]))
    assert len(one["cost"]) == 1 and len(four["cost"]) == 4
    assert abs(one["final_cost"] - ref[1]) <= 3e-7 + 1e-5 * abs(ref[1]), (one["final_cost"], ref)
    assert abs(four["final_cost"] - ref[4]) <= 0.02 * abs(ref[0]), (four["final_cost"], ref)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched():
    import smash_amd
    from smash_amd import _lib
    from smash_amd.solver import _pack
    from smash_amd import synth
    L = _lib.lib()
    name, mapping = mg.HYPER_CASES[0]
    g, z, setup, mesh, inp, par, sta, HP, HS = _case(name, mapping)
    desc = np.asfortranarray(inp.descriptor, dtype=np.float32)
    nd, nh = desc.shape[2], setup.optimize.nhyper
    hpm, hsm = HP.matrix(), HS.matrix()
    hpb, hsb = np.full((nh, 16), 7.0, np.float32, order="F"), np.full((nh, 8), 7.0, np.float32, order="F")
    planes_p, planes_s = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    for o, names in ((planes_p, synth.PARAM_NAMES), (planes_s, synth.STATE_NAMES)):
        for k in names:
            getattr(o, k)[...] = 7.0
    P, kp = _pack(planes_p, synth.PARAM_NAMES, _lib.Parameters)
    S, ks = _pack(planes_s, synth.STATE_NAMES, _lib.States)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def untouched():
        return (np.all(hpb == 7.0) and np.all(hsb == 7.0) and all(np.all(a == 7.0) for a in kp + ks)
                and hu.same_bits(hpm, HP.matrix()) and hu.same_bits(hsm, HS.matrix()))

    def all_calls(h, code, descriptors=False):
        if descriptors:
            assert L.smashx_hyper_set_descriptors(h, 1, nd, ptr(desc)) == code
        assert L.smashx_hyper_upload(h, ptr(hpm), ptr(hsm)) == code
        assert L.smashx_hyper_gradient(h, ptr(hpb), ptr(hsb)) == code
        assert L.smashx_hyper_fields(h, C.byref(P), C.byref(S)) == code
        assert untouched()

    def plain_solver(**kw):
        s = smash_amd.Solver(setup, mesh, **kw)
        s.set_forcing(inp.prcp, inp.pet)
        s.set_qobs(inp.qobs)
        return s

    # SMASHX_E_ARG: NULL plan; bad mapping; nd < 0; NULL matrices
    s = plain_solver()
    all_calls(None, _lib.E_ARG, descriptors=True)
    assert L.smashx_hyper_set_descriptors(s._h, 0, nd, ptr(desc)) == _lib.E_ARG
    assert L.smashx_hyper_set_descriptors(s._h, 3, nd, ptr(desc)) == _lib.E_ARG
    assert L.smashx_hyper_set_descriptors(s._h, 1, -1, ptr(desc)) == _lib.E_ARG
    assert L.smashx_hyper_upload(s._h, None, ptr(hsm)) == _lib.E_ARG and L.smashx_hyper_gradient(s._h, ptr(hpb), None) == _lib.E_ARG
    # SMASHX_E_STATE: no descriptors set (options set)
    s.set_options(setup.optimize)
    all_calls(s._h, _lib.E_STATE)
    # ... descriptors dropped again
    assert L.smashx_hyper_set_descriptors(s._h, 1, nd, ptr(desc)) == 0 and L.smashx_hyper_set_descriptors(s._h, 1, nd, None) == 0
    all_calls(s._h, _lib.E_STATE)
    # ... no options set
    s2 = plain_solver()
    assert L.smashx_hyper_set_descriptors(s2._h, 1, nd, ptr(desc)) == 0
    all_calls(s2._h, _lib.E_STATE)
    # ... no upload behind hyper_fields / hyper_gradient; then no adjoint sweep behind hyper_gradient
    assert L.smashx_hyper_set_descriptors(s._h, 1, nd, ptr(desc)) == 0
    assert L.smashx_hyper_fields(s._h, C.byref(P), C.byref(S)) == _lib.E_STATE and L.smashx_hyper_gradient(s._h, ptr(hpb), ptr(hsb)) == _lib.E_STATE
    assert L.smashx_hyper_upload(s._h, ptr(hpm), ptr(hsm)) == 0
    assert L.smashx_hyper_gradient(s._h, ptr(hpb), ptr(hsb)) == _lib.E_STATE
    s.sweep(False)
    assert L.smashx_hyper_gradient(s._h, ptr(hpb), ptr(hsb)) == _lib.E_STATE and untouched()
    s.sweep(True, 1.0)
    # ... new descriptors void the upload
    assert L.smashx_hyper_set_descriptors(s._h, 1, nd, ptr(np.asfortranarray(desc * np.float32(0.5)))) == 0
    assert L.smashx_hyper_gradient(s._h, ptr(hpb), ptr(hsb)) == _lib.E_STATE and untouched()
    # SMASHX_E_UNSUPPORTED: denormalize_forward; wjreg with a regulariser
    for edit in ("denorm", "jreg"):
        o = setup.copy().optimize
        if edit == "denorm":
            o.denormalize_forward = True
        else:
            o.jreg_fun, o.wjreg_fun, o.wjreg = ["prior"], [1.0], 0.5
        s3 = plain_solver()
        assert L.smashx_hyper_set_descriptors(s3._h, 1, nd, ptr(desc)) == 0
        s3.set_options(o)
        all_calls(s3._h, _lib.E_UNSUPPORTED)
    # ... a tiled plan: a rectangle, and an owner_mask of one part
    # (without gauges: a part of a decomposition only takes the gauges that lie in it)
    setup0 = smash_amd.SetupDT(nd, 0, structure=setup.structure, dt=setup.dt, ntime_step=setup.ntime_step)
    setup0.optimize.mapping, setup0.optimize.nhyper = setup.optimize.mapping, nh
    mesh0 = smash_amd.MeshDT(setup0, mesh.nrow, mesh.ncol, 0)
    mesh0.dx, mesh0.flwdir, mesh0.flwacc, mesh0.path, mesh0.active_cell = mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell
    for kw in (dict(tile=(0, mesh.nrow, 0, mesh.ncol // 2)), dict(owner_mask=np.ones((mesh.nrow, mesh.ncol), np.int32, order="F"))):
        s4 = smash_amd.Solver(setup0, mesh0, **kw)
        s4.set_options(setup0.optimize)
        all_calls(s4._h, _lib.E_UNSUPPORTED, descriptors=True)
    # the plan that went through all this still evaluates
    assert L.smashx_hyper_set_descriptors(s._h, 1, nd, ptr(desc)) == 0
    assert L.smashx_hyper_upload(s._h, ptr(hpm), ptr(hsm)) == 0
    s.sweep(True, 1.0)
    assert L.smashx_hyper_gradient(s._h, ptr(hpb), ptr(hsb)) == 0 and np.any(hpb != 7.0) and not hpb[:, 2].any()     # (beta: not read by gr-b)


# ---- 7. it pays -----------------------------------------------------------------------------------------------------------------------------------------
def test_one_device_evaluation_is_faster_than_one_host_evaluation():
    """256 x 256 x 48 steps, hyper-polynomial, nd = 4: one evaluation with the maps on the device against one through the host maps,
    wall time, median of 3 after one warm-up each"""
    import smash_amd
    from smash_amd import synth
    n, nt, nd = 256, 48, 4
    m = synth.make_mesh(n, n, ng=3)
    rng = np.random.default_rng(5)
    setup = smash_amd.SetupDT(nd, m.ng, structure="gr-b", dt=3600.0, ntime_step=nt)
    o = setup.optimize
    o.mapping, o.nhyper, o.jobs_fun, o.wjobs_fun = "hyper-polynomial", 1 + 2 * nd, ["nse"], [1.0]
    mesh = smash_amd.MeshDT.from_synth(setup, m)
    inp = smash_amd.Input_DataDT(setup, mesh)
    inp.prcp, inp.pet = synth.dense_forcing(m, nt)
    inp.qobs = np.asfortranarray((0.2 + 3.0 * rng.random((m.ng, nt))).astype(np.float32))
    desc = np.asfortranarray(rng.random((n, n, nd)).astype(np.float32))
    desc[0, 0, :], desc[1, 0, :] = 0.0, 1.0
    inp.descriptor = desc
    par, sta = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    from smash_amd.optimize import hyper_problem_initialise
    HP, HS, *_ = hyper_problem_initialise(setup, mesh, smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(n, n)),
                                          smash_amd.StatesDT.from_dict(mesh, synth.make_states(n, n, warm=True)))
    M = HP.matrix()
    M[1::2], M[2::2] = 0.1, 1.3
    HP.set_matrix(M)
    out = smash_amd.OutputDT(setup, mesh)
    sol = _solver(setup, mesh, inp)
    hpm, hsm = HP.matrix(), HS.matrix()

    def on_device():
        sol.hyper_upload(hpm, hsm)
        sol.sweep(True, 1.0)
        sol.cost_and_qsim(out)
        return sol.hyper_gradient()

    par_b, sta_b = par.copy(), sta.copy()

    def on_host():
        HPb, HSb = HP.copy(), HS.copy()
        smash_amd.hyper_forward_b(setup, mesh, inp, par, par_b, HP, HPb, HP, sta, sta_b, HS, HSb, HS, out, None, np.float32(0), np.float32(1))
        return HPb.matrix(), HSb.matrix()

    def median3(fn):
        fn()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[1], r

    t_dev, (hpb, hsb) = median3(on_device)
    t_host, (rpb, rsb) = median3(on_host)
    print(f"one evaluation at {n} x {n} x {nt}, hyper-polynomial nd = {nd}: device map {t_dev * 1e3:.1f} ms, host map {t_host * 1e3:.1f} ms",
          sol.hyper_info())
    assert hu.same_bits(hpb, rpb) and hu.same_bits(hsb, rsb)
    assert t_dev < t_host
