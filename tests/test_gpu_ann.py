"""GPU: the ANN regionalisation on the device (include/smashx_ann.h, smash_amd/csrc/sx_annmap.h) and smash_amd.ann_optimize over it.  The
oracle is the same network on the host (smashx_ann_host_*, csrc/sx_annhost.h: code the kernels do not run, pinned to the reference's
net.py by tests/test_ann_cpu.py); planes, costs and weight gradients are compared by their bits, and every check holds in both builds
(the default one and SMASHX_EXACT_LIBM=1).  The mesh is the masked D8 mesh of tests/test_gpu_hyper_device.py: 33 x 29, an active count
that is no multiple of 64, nt = 24."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import ann_util as au  # noqa: E402
import golden_util as gu  # noqa: E402
from test_gpu_hyper_device import _synth_case  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = -7.0


def _bounds(names, structure="gr-b"):
    """gr-b: the whole calibration box of the field; vic-a, whose run-time exponents leave the fp32 range at the corners of that box,
    and "narrow" (all 24 fields at once): 20 % around the values of the synthetic fields"""
    from smash_amd import synth
    from smash_amd.types import GLB_PARAMETERS, GLB_STATES, GUB_PARAMETERS, GUB_STATES
    P, S = synth.make_parameters(33, 29), synth.make_states(33, 29, warm=True)
    out = []
    for k in names:
        if structure in ("vic-a", "narrow"):
            v = np.asarray((P if k in synth.PARAM_NAMES else S)[k], np.float64)
            out.append((float(v.min()) - 0.2 * abs(float(v.min())), float(v.max()) + 0.2 * abs(float(v.max()))))
        elif k in synth.PARAM_NAMES:
            i = synth.PARAM_NAMES.index(k)
            out.append((float(GLB_PARAMETERS[i]), float(GUB_PARAMETERS[i])))
        else:
            i = synth.STATE_NAMES.index(k)
            out.append((float(GLB_STATES[i]), float(GUB_STATES[i])))
    return out


# name -> (structure, nd, control vector, specification of the net)
NETS = {
    "nd1_5_3": ("gr-b", 1, ("cp", "cft", "exc"), [(5, "relu"), (None, "sigmoid"), "scale"]),
    "cap_64_64": ("gr-b", 6, ("cp", "cft", "exc", "lr"), [(64, "relu"), (64, "tanh"), (None, "sigmoid"), "scale"]),
    "every_activation": ("gr-b", 2, ("cp", "lr", "hp"), [(7, ("elu", "tanh")), (6, ("selu", "leaky_relu")), (5, "relu"), (None, "sigmoid"), "scale"]),
    "no_scale": ("gr-b", 2, ("hp", "hft"), [(4, "tanh"), (None, "sigmoid")]),
    "unread_field": ("gr-b", 2, ("cp", "cst", "lr"), [(5, "relu"), (None, "sigmoid"), "scale"]),
    "vic_a": ("vic-a", 6, ("b", "cusl1", "ks", "husl1"), [(9, "elu"), (None, "sigmoid"), "scale"]),
    # exactly the device limit: 32 + 64 + 64 + 64 + 24 + 64 = 312 slots = 159 744 B of LDS per workgroup, four dense layers of the
    # widest kind, all 24 fields as outputs (most of which gr-b does not read)
    "limit_312": ("gr-b", 32, None, [(64, "relu"), (64, "tanh"), (64, "elu"), (None, "sigmoid"), "scale"]),
}


def _case(name):
    import smash_amd
    from smash_amd import synth
    structure, nd, cv, spec = NETS[name]
    narrow = cv is None
    if narrow:
        cv = tuple(synth.PARAM_NAMES) + tuple(synth.STATE_NAMES)
    setup, mesh, inp, _, _ = _synth_case(structure, "hyper-linear", min(nd, 6))
    if nd > 6:                                # more descriptors than that case plants its exact 0 and 1 for: drawn here, in [0, 1)
        inp.descriptor = np.asfortranarray(np.random.default_rng(nd).random((33, 29, nd), dtype=np.float32))
    par = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(33, 29))
    sta = smash_amd.StatesDT.from_dict(mesh, synth.make_states(33, 29, warm=True))
    net = au.build_net(smash_amd.Net, nd, spec, len(cv), _bounds(cv, "narrow" if narrow else structure), random_state=len(name))
    return setup, mesh, inp, par, sta, net, list(cv)


def _solver(setup, mesh, inp, par, sta, net=None, cv=None):
    from smash_amd.solver import _solver_for
    s = _solver_for(setup, mesh, inp)
    s.set_ann_descriptors(np.asfortranarray(inp.descriptor, dtype=np.float32))
    s.upload(par, sta)
    if net is not None:
        s.set_ann_net(net, cv)
    return s


def _filled(mesh):
    import smash_amd
    from smash_amd import synth
    p, s = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    for o, names in ((p, synth.PARAM_NAMES), (s, synth.STATE_NAMES)):
        for k in names:
            getattr(o, k)[...] = FILL
    return p, s


def _plane(p, s, k):
    from smash_amd import synth
    return getattr(p if k in synth.PARAM_NAMES else s, k)


def _gradient_with_span(sol, span=None):
    old = os.environ.pop("SMASHX_ANN_SPAN", None)
    try:
        if span is not None:
            os.environ["SMASHX_ANN_SPAN"] = str(span)
        return sol.ann_gradient()
    finally:
        os.environ.pop("SMASHX_ANN_SPAN", None)
        if old is not None:
            os.environ["SMASHX_ANN_SPAN"] = old


@pytest.mark.parametrize("name", list(NETS))
def test_one_evaluation_equals_the_host_composition(name):
    """upload -> ann_upload -> adjoint sweep -> ann_gradient against the host network around forward_b: the mapped planes, the cost,
    the discharge and the weight gradient bit for bit; the gradient again with the span forced short (at least 3 spans)"""
    import smash_amd
    from smash_amd import synth
    setup, mesh, inp, par, sta, net, cv = _case(name)
    (rr, cc), _ = au.column_major_cells(mesh.active_cell)
    act = np.asarray(mesh.active_cell) == 1
    x = np.ascontiguousarray(np.asarray(inp.descriptor, np.float32)[rr, cc])
    w = net.weights()
    if name == "cap_64_64":
        assert w.size > 64 * 64                                   # more than one wavefront of weight chains per stage
    if name == "limit_312":
        assert len(cv) == 24 and net.graph()[0] + sum(l.neurons for l in net._dense()) + 64 == 312

    sol = _solver(setup, mesh, inp, par, sta, net, cv)
    sol.ann_upload(w)
    p, s = _filled(mesh)
    sol.ann_fields(p, s)
    y = net._forward_pass(x)
    assert np.all(np.isfinite(y)) and y.std() > 0
    for i, k in enumerate(cv):
        assert au.same_bits(_plane(p, s, k)[rr, cc], y[:, i]), k
        assert np.all(_plane(p, s, k)[~act] == FILL), k           # inactive cells are left as the caller had them
    for k in list(synth.PARAM_NAMES) + list(synth.STATE_NAMES):
        if k not in cv:
            assert np.all(_plane(p, s, k) == FILL), k             # ... and so is every other field

    out = smash_amd.OutputDT(setup, mesh)
    sol.sweep(True, 1.0)
    cost = sol.cost_and_qsim(out)
    wb = sol.ann_gradient()
    info = sol.ann_info()
    assert info["nweights"] == w.size and info["span"] >= sol.ncells and info["nd"] == x.shape[1]
    if name == "limit_312":
        assert info["lds_bytes"] == 312 * 512 == 159744
    short = 128
    assert -(-sol.ncells // short) >= 3
    wb_short = _gradient_with_span(sol, short)
    assert sol.ann_info()["span"] == short
    assert au.same_bits(wb_short, wb)

    # the host composition: the host network's planes through forward_b, its gradient planes through the host network's adjoint
    hp, hs = par.copy(), sta.copy()
    for i, k in enumerate(cv):
        _plane(hp, hs, k)[rr, cc] = y[:, i]
    hout = smash_amd.OutputDT(setup, mesh)
    par_b, sta_b = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    hcost = smash_amd.forward_b(setup, mesh, inp, hp, par_b, hp, par_b, hs, sta_b, hs, sta_b, hout, None, np.float32(0), np.float32(1))
    assert np.isfinite(cost) and au.same_bits(np.float32(cost), np.float32(hcost))
    assert au.same_bits(np.asarray(out.qsim, np.float32), np.asarray(hout.qsim, np.float32))
    loss_grad = np.stack([np.asarray(_plane(par_b, sta_b, k), np.float32)[rr, cc] for k in cv], axis=1)
    if name == "unread_field":
        assert not loss_grad[:, 1].any() and loss_grad[:, 0].any()
    ref = net.gradient(x, loss_grad)
    assert np.all(np.isfinite(ref)) and np.any(ref != 0)
    assert au.same_bits(wb, ref)


def test_ann_optimize_device_equals_host_composition():
    """three epochs of ann_optimize with the maps on the device and through the host composition: the same loss_train, weights and
    planes, bit for bit; the caller's descriptors come back as they were"""
    import smash_amd
    runs = {}
    for device_map in (True, False):
        setup, mesh, inp, par, sta, net, cv = _case("every_activation")
        inp.descriptor = np.asfortranarray(inp.descriptor * np.float32(37.5) + np.float32(3.0))     # in their own units: normalised inside
        before = inp.descriptor.copy(order="F")
        out = smash_amd.OutputDT(setup, mesh)
        net = smash_amd.ann_optimize(setup, mesh, inp, par, sta, out, cv, _bounds(cv), net=net, epochs=3, early_stopping=True,
                                     device_map=device_map)
        assert au.same_bits(inp.descriptor, before)
        runs[device_map] = (net, par, sta, out)
    (nd_, pd_, sd_, od_), (nh_, ph_, sh_, oh_) = runs[True], runs[False]
    assert len(nd_.history["loss_train"]) == 3 and nd_.history["loss_train"] == nh_.history["loss_train"]
    assert au.same_bits(nd_.weights(), nh_.weights())
    for k in cv:
        a, b = _plane(pd_, sd_, k), _plane(ph_, sh_, k)
        assert au.same_bits(np.asarray(a, np.float32), np.asarray(b, np.float32)), k
    assert au.same_bits(np.asarray(od_.qsim, np.float32), np.asarray(oh_.qsim, np.float32))


def test_host_composition_regularises_against_the_fields_before_the_training():
    """device_map = False with a prior regulariser: the background of every epoch is the fields as they were before the training
    (_ann_optimize.py:74-75), so the jreg term is positive as soon as the network has moved them; the device path refuses"""
    import smash_amd
    from smash_amd import _lib
    setup, mesh, inp, par, sta, net, cv = _case("nd1_5_3")
    o = setup.optimize
    o.jreg_fun, o.wjreg_fun, o.wjreg = ["prior"], [1.0], 0.5
    out = smash_amd.OutputDT(setup, mesh)
    before = par.cp.copy()
    smash_amd.ann_optimize(setup, mesh, inp, par, sta, out, cv, _bounds(cv), net=net, epochs=2, device_map=False)
    assert not np.array_equal(par.cp, before)
    assert out.cost_jreg > 0 and np.isfinite(out.cost) and abs(out.cost - (out.cost_jobs + 0.5 * out.cost_jreg)) <= 1e-5 * abs(out.cost)
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.ann_optimize(setup, mesh, inp, par, sta, out, cv, _bounds(cv), net=net, epochs=1, device_map=True)
    assert e.value.code == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("case", list(au.FIT_CASES))
def test_ann_optimize_follows_the_reference(case):
    """both paths against tests/golden/ann/fit_*.npz.  On the exact-libm build, whose sweep is the reference's bit for bit, with the
    bars of tests/test_ann_cpu.py; on the default build, whose sweep follows the reference to rounding only, the two paths are held
    to each other bit for bit and the losses are printed beside the recorded ones"""
    from smash_amd import _lib
    import test_ann_cpu as tc
    dev, host = tc.run_fit(case, device_map=True), tc.run_fit(case, device_map=False)
    assert dev["loss_train"] == host["loss_train"] and au.same_bits(dev["weights"], host["weights"])
    for k in au.FIT_CONTROL:
        assert au.same_bits(dev["planes"][k], host["planes"][k]), k
    if _lib.EXACT:
        tc.check_fit(case, dev)
    else:
        print(case, "loss_train", dev["loss_train"], "reference", list(au.fixture("fit_" + case)["loss_train"]))


def test_refusals_leave_the_buffers_untouched():
    import smash_amd
    from smash_amd import _lib, synth
    from smash_amd.solver import Solver
    L = _lib.lib()
    setup, mesh, inp, par, sta, net, cv = _case("nd1_5_3")
    desc = np.asfortranarray(inp.descriptor, dtype=np.float32)
    w = net.weights()
    nd, kind, width, ncv, lower, upper = net.graph()
    field = smash_amd.check_ann_control_vector(cv, ncv)
    wb = np.full(w.size, FILL)
    P, S = _lib.Parameters(), _lib.States()
    p, s = _filled(mesh)
    for k in ("cp", "cft", "exc"):
        P.f[synth.PARAM_NAMES.index(k)] = getattr(p, k).ctypes.data

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def untouched():
        return np.all(wb == FILL) and all(np.all(getattr(p, k) == FILL) for k in ("cp", "cft", "exc"))

    from smash_amd.solver import _solver_for
    sol = _solver_for(setup, mesh, inp)
    h = sol._h
    set_net = lambda k=kind, wd=width, n=ncv, f=field, lo=lower, up=upper, nl=None: L.smashx_ann_set_net(  # noqa: E731
        h, len(k) if nl is None else nl, ptr(k), ptr(wd), n, ptr(f), ptr(lo), ptr(up))
    # E_ARG
    assert L.smashx_ann_set_descriptors(h, 1, None) == _lib.E_ARG and L.smashx_ann_set_descriptors(None, 1, ptr(desc)) == _lib.E_ARG
    assert L.smashx_ann_set_descriptors(h, 0, ptr(desc)) == _lib.E_ARG
    assert L.smashx_ann_upload(h, None) == _lib.E_ARG and L.smashx_ann_gradient(h, None) == _lib.E_ARG
    assert L.smashx_ann_fields(None, None, None) == _lib.E_ARG and L.smashx_ann_info(h, None, None) == _lib.E_ARG
    assert L.smashx_ann_set_net(h, len(kind), None, ptr(width), ncv, ptr(field), ptr(lower), ptr(upper)) == _lib.E_ARG
    assert L.smashx_ann_set_net(h, len(kind), ptr(kind), None, ncv, ptr(field), ptr(lower), ptr(upper)) == _lib.E_ARG
    assert L.smashx_ann_set_net(h, len(kind), ptr(kind), ptr(width), ncv, None, ptr(lower), ptr(upper)) == _lib.E_ARG
    # E_STATE: nothing set yet
    assert L.smashx_ann_upload(h, ptr(w)) == _lib.E_STATE                                       # no descriptors
    assert set_net() == _lib.E_STATE                                                            # the net's input width is theirs
    assert L.smashx_ann_set_descriptors(h, 1, ptr(desc)) == 0
    assert L.smashx_ann_upload(h, ptr(w)) == _lib.E_STATE                                       # no net
    bad_kind = kind.copy(); bad_kind[1] = 99
    bad_field = field.copy(); bad_field[0] = 24
    twice = field.copy(); twice[1] = twice[0]
    bad_width = width.copy(); bad_width[1] += 1
    last = width.copy(); last[-3:] += 1
    assert L.smashx_ann_set_net(h, len(kind), ptr(kind), ptr(width), ncv, ptr(field), None, ptr(upper)) == _lib.E_ARG      # a scale layer, no bounds
    assert L.smashx_ann_set_net(h, len(kind), ptr(kind), ptr(width), ncv, ptr(field), ptr(lower), None) == _lib.E_ARG
    for kw in (dict(k=bad_kind), dict(f=bad_field), dict(f=twice), dict(wd=bad_width), dict(wd=last), dict(k=kind[1:], wd=width[1:], nl=len(kind) - 1)):
        assert set_net(**kw) == _lib.E_ARG, kw
    # E_UNSUPPORTED: the layer kinds and sizes outside the contract
    for refused in ("softplus", "softmax", "dropout"):
        k2 = kind.copy(); k2[1] = _lib.ANN_LAYER[refused]
        assert set_net(k=k2) == _lib.E_UNSUPPORTED, refused
    wide = width.copy(); wide[0] = wide[1] = 65
    assert set_net(wd=wide) == _lib.E_UNSUPPORTED
    deep_k = np.array([1, 2] * 5 + list(kind[2:]), np.int32)
    deep_w = np.array([5] * 10 + list(width[2:]), np.int32)
    assert set_net(k=deep_k, wd=deep_w) == _lib.E_UNSUPPORTED                                   # five dense layers
    k25, w25, f25 = np.array([1], np.int32), np.array([25], np.int32), np.arange(25, dtype=np.int32)
    assert L.smashx_ann_set_net(h, 1, ptr(k25), ptr(w25), 25, ptr(f25), None, None) == _lib.E_UNSUPPORTED      # ncv > 24
    # the LDS rows: 150 descriptors in front of (64, 64, ncv) are 150 + 64 + 64 + 3 + 64 = 345 > 312
    many = np.asfortranarray(np.random.default_rng(4).random((mesh.nrow, mesh.ncol, 150), dtype=np.float32))
    assert L.smashx_ann_set_descriptors(h, 150, ptr(many)) == 0
    rows_k, rows_w = np.array([1, 2, 1, 2] + list(kind[2:]), np.int32), np.array([64] * 4 + list(width[2:]), np.int32)
    assert set_net(k=rows_k, wd=rows_w) == _lib.E_UNSUPPORTED
    rows_w[:4] = 20                                                                             # 150 + 20 + 20 + 3 + 20 = 213: taken
    assert set_net(k=rows_k, wd=rows_w) == 0
    assert L.smashx_ann_set_descriptors(h, 1, ptr(desc)) == 0
    assert L.smashx_ann_upload(h, ptr(w)) == _lib.E_STATE                                       # that net's input width is not 1
    assert set_net() == 0
    # E_STATE: no smashx_upload; then no adjoint sweep behind the ann_upload; then new descriptors / a new net since the upload
    fresh = Solver(setup, mesh)
    assert L.smashx_ann_set_descriptors(fresh._h, 1, ptr(desc)) == 0
    assert L.smashx_ann_set_net(fresh._h, len(kind), ptr(kind), ptr(width), ncv, ptr(field), ptr(lower), ptr(upper)) == 0
    assert L.smashx_ann_upload(fresh._h, ptr(w)) == _lib.E_STATE
    fresh.close()
    sol.upload(par, sta)
    assert L.smashx_ann_gradient(h, ptr(wb)) == _lib.E_STATE and L.smashx_ann_fields(h, C.byref(P), C.byref(S)) == _lib.E_STATE
    sol.sweep(True, 1.0)                                                                         # an adjoint sweep, but behind no ann_upload
    assert L.smashx_ann_gradient(h, ptr(wb)) == _lib.E_STATE
    assert L.smashx_ann_upload(h, ptr(w)) == 0
    assert L.smashx_ann_gradient(h, ptr(wb)) == _lib.E_STATE                                     # the sweep lies before the upload
    sol.sweep(False)
    assert L.smashx_ann_gradient(h, ptr(wb)) == _lib.E_STATE                                     # a forward sweep
    r0, c0 = (int(v[0]) for v in np.nonzero(np.asarray(mesh.active_cell) == 1))                  # an active cell: the plan keeps no others
    other = desc.copy(order="F"); other[r0, c0, 0] += np.float32(0.25)
    assert L.smashx_ann_set_descriptors(h, 1, ptr(other)) == 0
    assert L.smashx_ann_fields(h, C.byref(P), C.byref(S)) == _lib.E_STATE                        # new descriptors since the upload
    assert L.smashx_ann_set_descriptors(h, 1, ptr(desc)) == 0 and L.smashx_ann_upload(h, ptr(w)) == 0
    assert L.smashx_ann_set_descriptors(h, 1, ptr(desc)) == 0                                    # the same contents: nothing changes
    assert L.smashx_ann_fields(h, C.byref(P), C.byref(S)) == 0 and np.all(p.cp[np.asarray(mesh.active_cell) == 1] != FILL)
    p.cp[...] = FILL; p.cft[...] = FILL; p.exc[...] = FILL
    assert set_net() == 0
    assert L.smashx_ann_fields(h, C.byref(P), C.byref(S)) == _lib.E_STATE                        # a new net since the upload
    assert untouched()
    # E_UNSUPPORTED: a regulariser (the jreg term does not see the mapped fields)
    o = setup.copy().optimize
    o.jreg_fun, o.wjreg_fun, o.wjreg = ["prior"], [1.0], 0.5
    o.optim_parameters = np.array([int(k in cv) for k in synth.PARAM_NAMES], np.int32)
    reg = Solver(setup, mesh)
    reg.set_forcing(inp.prcp, inp.pet)
    reg.set_qobs(inp.qobs)
    reg.set_options(o)
    assert L.smashx_ann_set_descriptors(reg._h, 1, ptr(desc)) == 0
    assert L.smashx_ann_set_net(reg._h, len(kind), ptr(kind), ptr(width), ncv, ptr(field), ptr(lower), ptr(upper)) == 0
    reg.upload(par, sta, par, sta)
    assert L.smashx_ann_upload(reg._h, ptr(w)) == _lib.E_UNSUPPORTED and L.smashx_ann_gradient(reg._h, ptr(wb)) == _lib.E_UNSUPPORTED
    assert L.smashx_ann_fields(reg._h, C.byref(P), C.byref(S)) == _lib.E_UNSUPPORTED
    reg.close()
    assert untouched()
    # E_UNSUPPORTED: a tiled plan -- a rectangle, and an owner mask of one part (without gauges: a part only takes the gauges in it)
    setup0 = smash_amd.SetupDT(1, 0, structure=setup.structure, dt=setup.dt, ntime_step=setup.ntime_step)
    mesh0 = smash_amd.MeshDT(setup0, mesh.nrow, mesh.ncol, 0)
    mesh0.dx, mesh0.flwdir, mesh0.flwacc, mesh0.path, mesh0.active_cell = mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell
    for kw in (dict(tile=(0, mesh.nrow, 0, mesh.ncol // 2)), dict(owner_mask=np.ones((mesh.nrow, mesh.ncol), np.int32, order="F"))):
        tiled = Solver(setup0, mesh0, **kw)
        assert L.smashx_ann_set_descriptors(tiled._h, 1, ptr(desc)) == _lib.E_UNSUPPORTED
        assert L.smashx_ann_set_net(tiled._h, len(kind), ptr(kind), ptr(width), ncv, ptr(field), ptr(lower), ptr(upper)) == _lib.E_UNSUPPORTED
        assert L.smashx_ann_upload(tiled._h, ptr(w)) == _lib.E_UNSUPPORTED and L.smashx_ann_gradient(tiled._h, ptr(wb)) == _lib.E_UNSUPPORTED
        assert L.smashx_ann_fields(tiled._h, C.byref(P), C.byref(S)) == _lib.E_UNSUPPORTED
        tiled.close()
    assert untouched()
    # the plan still evaluates
    out = smash_amd.OutputDT(setup, mesh)
    sol.set_ann_net(net, cv)
    sol.ann_upload(w)
    sol.sweep(True, 1.0)
    assert np.isfinite(sol.cost_and_qsim(out))
    g = sol.ann_gradient()
    assert np.all(np.isfinite(g)) and np.any(g != 0)
