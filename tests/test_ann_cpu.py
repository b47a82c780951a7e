"""CPU: the ANN regionalisation as far as it goes without a GPU -- include/smashx_ann.h against the binding, the exported symbols, the
argument checks of the Python layer, the host network (smashx_ann_host_*, csrc/sx_ann.h + sx_annhost.h) and smash_amd.Net against what
the reference's own net.py computes (tests/golden/ann/net_functions.npz, tests/golden/make_ann.py), the shared exp against the host
libm, and smash_amd.ann_optimize, driven through the injectable evaluation by the CPU oracle (oracle/pyoracle.py, pinned to the
reference bit for bit), against the recorded trainings tests/golden/ann/fit_*.npz."""
import ctypes as C
import ctypes.util
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ann_util as au  # noqa: E402
import golden_util as gu  # noqa: E402
import hyper_device_util as hu  # noqa: E402
from oracle import pyoracle  # noqa: E402

ANN_HEADER = os.path.join(ROOT, "include", "smashx_ann.h")
NAMES = ["smashx_ann_set_descriptors", "smashx_ann_set_net", "smashx_ann_upload", "smashx_ann_gradient", "smashx_ann_fields",
         "smashx_ann_info", "smashx_ann_host_nweights", "smashx_ann_host_forward", "smashx_ann_host_gradient",
         "smashx_ann_host_activation", "smashx_ann_host_exp"]
RTOL = 1e-12      # fp64 eps 1.1e-16 over chains of <~ 100 operations, with 100 x margin


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_ann_header_matches_the_binding():
    """include/smashx_ann.h against _lib.ANN_PROTOTYPES and _lib.ANN_LAYER with the parser and the type rules tests/test_abi_header_cpu.py
    applies to smashx.h; counts taken from the header's own text, so that a declaration the parser skips fails here"""
    import test_abi_header_cpu as ah
    from smash_amd import _lib
    text = open(ANN_HEADER).read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    enum = {k: v for k, v in h["constants"].items() if k != "SMASHX_ANN_H"}
    assert {k: int(v) for k, v in enum.items()} == {"SMASHX_ANN_" + k.upper(): v for k, v in _lib.ANN_LAYER.items()}
    assert re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", ah.strip(text)[0], flags=re.M) == ["SMASHX_ANN_H"]
    assert not re.search(r"\b(struct|typedef)\b", ah.strip(text)[1])
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == len(NAMES)
    assert list(h["functions"]) == NAMES == list(_lib.ANN_PROTOTYPES) == _lib.ANN_SYMBOLS
    others = (set(_lib.PROTOTYPES) | set(_lib.SETUP_PROTOTYPES) | set(_lib.FORCING_PROTOTYPES) | set(_lib.PRCP_PROTOTYPES)
              | set(_lib.SIGNATURE_PROTOTYPES) | set(_lib.HYPER_DEVICE_PROTOTYPES))
    assert not set(_lib.ANN_PROTOTYPES) & others
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.ANN_PROTOTYPES[name]
        assert not rptr and restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert [p[:3] for p in h["functions"]["smashx_ann_set_descriptors"][1]] == [
        ("plan", "smashx_plan", True), ("nd", "int", False), ("descriptor", "float", True)]
    assert [p[:3] for p in h["functions"]["smashx_ann_gradient"][1]] == [("plan", "smashx_plan", True), ("weights_b", "double", True)]
    # the comparison bites: a parameter turned into a pointer is reported
    flat = ah.parse(text.replace("smashx_plan* plan, int nd,", "smashx_plan* plan, int* nd,"))
    ah.check_type("nd", _lib.ANN_PROTOTYPES["smashx_ann_set_descriptors"][1][1],
                  *flat["functions"]["smashx_ann_set_descriptors"][1][1][1:], flat, _lib, findings, param=True)
    assert findings and "nd" in findings[0]


def test_smashx_h_brings_the_ann_header_along():
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    assert hdr.count('#include "smashx_ann.h"') == 1
    assert hdr.index('#include "smashx_hyper.h"') < hdr.index('#include "smashx_ann.h"')
    assert "#define SMASHX_ABI_VERSION 9" in hdr


def test_symbols_are_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        restype, argtypes = _lib.ANN_PROTOTYPES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.smashx_abi_sizes(None) == 9
    # the argument checks that need no plan
    assert L.smashx_ann_set_descriptors(None, 1, None) == _lib.E_ARG
    assert L.smashx_ann_set_net(None, 0, None, None, 0, None, None, None) == _lib.E_ARG
    assert L.smashx_ann_upload(None, None) == _lib.E_ARG and L.smashx_ann_gradient(None, None) == _lib.E_ARG
    assert L.smashx_ann_fields(None, None, None) == _lib.E_ARG and L.smashx_ann_info(None, None, None) == _lib.E_ARG
    kind, width = np.array([1, 6], np.int32), np.array([3, 3], np.int32)
    assert L.smashx_ann_host_nweights(2, 2, _ptr(kind), _ptr(width), 3) == 9
    assert L.smashx_ann_host_nweights(0, 2, _ptr(kind), _ptr(width), 3) == _lib.E_ARG
    assert L.smashx_ann_host_nweights(2, 2, _ptr(kind), _ptr(width), 4) == _lib.E_ARG
    assert L.smashx_ann_host_nweights(2, 2, None, _ptr(width), 3) == _lib.E_ARG
    for refused in ("softplus", "softmax", "dropout"):
        k2 = np.array([1, _lib.ANN_LAYER[refused]], np.int32)
        assert L.smashx_ann_host_nweights(2, 2, _ptr(k2), _ptr(width), 3) == _lib.E_UNSUPPORTED
    assert L.smashx_ann_host_activation(1, 0, None, None, None) == _lib.E_ARG and L.smashx_ann_host_exp(1, None, None) == _lib.E_ARG


# ---- argument checks of the Python layer ------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    import smash_amd
    from smash_amd import _lib
    good = np.zeros((5, 4, 2), np.float32, order="F")
    assert smash_amd.check_ann_descriptors(5, 4, good) == (2, good)
    for d in (None, good.astype(np.float64), np.ascontiguousarray(good), np.zeros((4, 5, 2), np.float32, order="F"), good[:, :, 0],
              np.zeros((5, 4, 0), np.float32, order="F"), good.tolist()):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.check_ann_descriptors(5, 4, d)
        assert e.value.code == _lib.E_ARG
    assert list(smash_amd.check_ann_control_vector(["cp", "hlr", "ci"], 3)) == [1, 16 + 7, 0]
    for cv, n in ((["cp", "cp"], 2), (["cp", "nope"], 2), (["cp"], 2)):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.check_ann_control_vector(cv, n)
        assert e.value.code == _lib.E_ARG
    w = np.zeros(7)
    assert smash_amd.check_ann_weights(7, w) is w
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.check_ann_weights(None, w)
    assert e.value.code == _lib.E_STATE
    ro = w.copy()
    ro.flags.writeable = False
    assert smash_amd.check_ann_weights(7, ro) is ro
    for a, wr in ((w[:6], False), (w.astype(np.float32), False), (np.zeros(14)[::2], False), (None, False), (ro, True)):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.check_ann_weights(7, a, writeable=wr)
        assert e.value.code == _lib.E_ARG
    # the graph of a Net as the C call takes it
    net = au.build_net(smash_amd.Net, 2, [(5, "relu"), (None, ("sigmoid",)), "scale"], 3, [(0, 1), (2, 3), (4, 5)])
    nd, kind, width, ncv, lower, upper = net.graph()
    assert (nd, ncv, list(kind), list(width)) == (2, 3, [1, 2, 1, 6, 8], [5, 5, 3, 3, 3])
    assert list(lower) == [0, 2, 4] and list(upper) == [1, 3, 5] and net.weights().size == 15 + 18
    with pytest.raises(ValueError):
        smash_amd.Net().compile()
    with pytest.raises(TypeError):
        smash_amd.Net().add("dense", {"neurons": 3})
    with pytest.raises(ValueError):
        smash_amd.Net().add("conv", {})
    with pytest.raises(KeyError):
        smash_amd.Net().add("dense", {"input_shape": (2,), "neurons": 3, "units": 1})
    # a layer outside the contract can be declared, as in the reference, and is refused when the network is evaluated
    drop = smash_amd.Net()
    drop.add("dense", {"input_shape": (2,), "neurons": 3})
    drop.add("dropout", {"drop_rate": 0.1})
    drop.compile()
    with pytest.raises(smash_amd.SmashxError) as e:
        drop._forward_pass(np.zeros((4, 2), np.float32))
    assert e.value.code == _lib.E_UNSUPPORTED


# ---- the host network against the reference's net.py ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fun():
    return au.fixture("net_functions")


@pytest.mark.parametrize("name", au.ACTIVATIONS)
def test_activation_and_gradient(fun, name):
    from smash_amd import _lib
    x = np.ascontiguousarray(fun[f"act_{name}_x"])
    y, dy = np.zeros_like(x), np.zeros_like(x)
    _lib.check(_lib.lib().smashx_ann_host_activation(_lib.ANN_LAYER[name], x.size, _ptr(x), _ptr(y), _ptr(dy)))
    assert _close(y, fun[f"act_{name}_y"]) and _close(dy, fun[f"act_{name}_dy"])
    assert np.any(y != 0) and np.any(dy != 0) and x.size >= 32
    # 1e-6 <= |x| < 0.01, where elu and selu subtract 1 from exp(x) and a relative bar would measure that cancellation: an ABSOLUTE
    # bar instead.  Both exps are within 1 ulp of exp(x) ~ 1, so they differ by at most 2 x 2.2e-16; the factor behind the
    # subtraction is at most selu's alpha x scale = 1.76, the further roundings are of numbers below 1: 2e-15 covers it twice over.
    xs = np.ascontiguousarray(fun[f"act_{name}_xs"])
    ys, dys = np.zeros_like(xs), np.zeros_like(xs)
    _lib.check(_lib.lib().smashx_ann_host_activation(_lib.ANN_LAYER[name], xs.size, _ptr(xs), _ptr(ys), _ptr(dys)))
    assert xs.size == 48 and np.abs(xs).max() < 0.01 and np.abs(xs).min() >= 1e-6
    print(name, "small |x|: max abs difference", float(np.abs(ys - fun[f"act_{name}_ys"]).max()), float(np.abs(dys - fun[f"act_{name}_dys"]).max()))
    assert np.abs(ys - fun[f"act_{name}_ys"]).max() <= 2e-15 and np.abs(dys - fun[f"act_{name}_dys"]).max() <= 2e-15


@pytest.mark.parametrize("name", au.OPTIMIZERS)
def test_optimizer_updates(fun, name):
    from smash_amd import net as sn
    opt = sn.OPT_FUNC[name](**({"momentum": 0.3} if name == "sgd" else {}))
    w1 = opt.update(fun[f"opt_{name}_w0"], fun[f"opt_{name}_g1"])
    w2 = opt.update(w1, fun[f"opt_{name}_g2"])
    assert _close(w1, fun[f"opt_{name}_w1"]) and _close(w2, fun[f"opt_{name}_w2"])
    assert not np.array_equal(w1, fun[f"opt_{name}_w0"])


def test_forward_and_backward_pass(fun):
    import smash_amd
    net = smash_amd.Net()
    net.add("dense", {"input_shape": (2,), "neurons": 3, "bias_initializer": "normal"})
    net.add("activation", {"name": "tanh"})
    net.add("dense", {"neurons": 2, "bias_initializer": "normal"})
    net.add("activation", {"name": "sigmoid"})
    net.add("scale", {"bounds": [(1.0, 9.0), (-3.0, 2.0)]})
    net.compile("sgd", random_state=7)
    assert au.same_bits(net.weights(), fun["pass_weights"])
    y = net._forward_pass(fun["pass_x"])
    assert y.dtype == np.float32 and au.same_bits(y, fun["pass_y"].astype(np.float32))          # fp64 inside, rounded once
    assert _close(net.gradient(fun["pass_x"], fun["pass_loss_grad"]), fun["pass_weights_b"])
    before = net.weights()
    net._backward_pass(fun["pass_loss_grad"], fun["pass_x"])
    assert _close(net.weights(), before - 0.01 * fun["pass_weights_b"])                          # sgd, learning_rate 0.01, no momentum
    frozen = net.copy()
    frozen.set_trainable([False, True, True, True, True])
    frozen._backward_pass(fun["pass_loss_grad"], fun["pass_x"])
    assert np.array_equal(frozen.weights()[:9], net.weights()[:9]) and not np.array_equal(frozen.weights()[9:], net.weights()[9:])


@pytest.mark.parametrize("init", ["glorot_uniform", "he_normal", "zeros"])
def test_initial_weights_bit_for_bit(fun, init):
    import smash_amd
    net = smash_amd.Net()
    net.add("dense", {"input_shape": (4,), "neurons": 6, "kernel_initializer": init, "bias_initializer": init})
    net.add("activation", {"name": "relu"})
    net.add("dense", {"neurons": 3, "kernel_initializer": init})
    net.compile("adam", random_state=au.FIT_SEED)
    assert au.same_bits(net.weights(), fun["init_" + init])
    assert (init == "zeros") == (not net.weights().any())


def test_shared_exp_against_the_host_libm():
    """sx_ann_exp against exp of the C library at 400001 evenly spaced points of [-708, 709], 1000000 uniform draws of the same interval
    (seed 1) and 200000 of [-2, 2], plus +-0, +-inf and NaN.  Measured maximum distance: 1 ulp (mean 0.11); the bar is 2 ulp."""
    from smash_amd import _lib
    rng = np.random.default_rng(1)
    x = np.concatenate([np.linspace(-708.0, 709.0, 400001), rng.uniform(-708.0, 709.0, 1000000), rng.uniform(-2.0, 2.0, 200000)])
    y = np.zeros_like(x)
    _lib.check(_lib.lib().smashx_ann_host_exp(x.size, _ptr(x), _ptr(y)))
    lm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lm.exp.restype, lm.exp.argtypes = C.c_double, [C.c_double]
    sample = np.concatenate([np.arange(0, x.size, 37), np.argsort(x)[:2000], np.argsort(x)[-2000:]])      # libm one call at a time: a subset,
    ref = np.array([lm.exp(float(v)) for v in x[sample]])                                               # numpy's exp over all of it below
    ulp = np.abs(y[sample].view(np.int64) - ref.view(np.int64))
    ulp_np = np.abs(y.view(np.int64) - np.exp(x).view(np.int64))
    print("max ulp distance: libm", int(ulp.max()), "numpy", int(ulp_np.max()))
    assert ulp.max() <= 2 and ulp_np.max() <= 2
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    ys = np.zeros_like(sp)
    _lib.check(_lib.lib().smashx_ann_host_exp(sp.size, _ptr(sp), _ptr(ys)))
    assert list(ys[:4]) == [1.0, 1.0, np.inf, 0.0] and np.isnan(ys[4]) and not np.signbit(ys[3])


# ---- the training --------------------------------------------------------------------------------------------------------------------------------
def run_fit(case, device_map=None):
    """ann_optimize on the recorded case: device_map None -> the CPU oracle as the evaluation; True / False -> the GPU paths"""
    import smash_amd
    from smash_amd import synth
    spec, optimizer, options, epochs, early = au.FIT_CASES[case]
    g, z, setup, mesh, inp, par, sta, out = hu.calibration_case("hyper-linear", 0)
    setup.optimize.optim_parameters = np.zeros(16, np.int32)
    before = inp.descriptor.copy(order="F")
    net = None
    if spec is not None:
        net = au.build_net(smash_amd.Net, before.shape[2], spec, len(au.FIT_CONTROL), au.FIT_BOUNDS, optimizer, options, au.FIT_SEED, bias="zeros")
    seen = []

    def evaluate(planes):
        p, s = dict(g.params), dict(g.states)
        p.update({k: np.asfortranarray(v, dtype=np.float32) for k, v in planes.items()})
        seen.append((float(inp.descriptor.min()), float(inp.descriptor.max())))
        r = pyoracle.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, p, s, adjoint=True, jobs_fun=("nse",), wjobs_fun=(1.0,))
        return r["cost"], r["parameters_b"]

    net = smash_amd.ann_optimize(setup, mesh, inp, par, sta, out, list(au.FIT_CONTROL), au.FIT_BOUNDS, net=net, optimizer=optimizer,
                                 learning_rate=options["learning_rate"], epochs=epochs, early_stopping=early, random_state=au.FIT_SEED,
                                 evaluate=evaluate if device_map is None else None, device_map=bool(device_map))
    assert hu.same_bits(inp.descriptor, before)                  # the caller's descriptors, bit for bit
    assert all(lo == 0.0 and hi == 1.0 for lo, hi in seen)       # the training saw them normalised over the whole grid
    o = setup.optimize
    assert [int(v) for v in o.optim_parameters] == [int(k in au.FIT_CONTROL) for k in synth.PARAM_NAMES]
    return dict(net=net, loss_train=list(net.history["loss_train"]), weights=net.weights(),
                planes={k: np.asarray(getattr(par, k), np.float32) for k in au.FIT_CONTROL}, epochs=epochs)


def check_fit(case, run):
    z = au.fixture("fit_" + case)
    assert len(run["loss_train"]) == run["epochs"] == len(z["loss_train"])
    e_loss, e_w = gu.rel_l2(np.array(run["loss_train"]), z["loss_train"]), gu.rel_l2(run["weights"], z["weights"])
    cells = sum(int(np.count_nonzero(run["planes"][k] != z["plane_" + k])) for k in au.FIT_CONTROL)
    total = sum(z["plane_" + k].size for k in au.FIT_CONTROL)
    print(case, "loss_train rel L2", e_loss, "weights rel L2", e_w, "plane cells that differ", cells, "of", total)
    assert e_loss <= gu.tol(float(z["noise_loss"]), base=1e-9) and e_w <= gu.tol(float(z["noise_weights"]), base=1e-9)
    assert cells <= total // 10000                                # at most 1 cell in 10^4 differs at all ...
    for k in au.FIT_CONTROL:                                      # ... and none by more than one fp32 ulp
        a, b = run["planes"][k], np.asarray(z["plane_" + k], np.float32)
        assert np.all(np.abs(a - b) <= np.spacing(np.abs(b))), k


@pytest.mark.parametrize("case", list(au.FIT_CASES))
def test_ann_optimize_over_the_oracle_follows_the_reference(case):
    run = run_fit(case)
    z = au.fixture("fit_" + case)
    if au.FIT_CASES[case][0] is None:
        # the auto-graph rule and the draws of compile(random_state): the initial weights of the reference, bit for bit
        import smash_amd
        n = int(np.count_nonzero(np.asarray(hu.calibration_case("hyper-linear", 0)[3].active_cell) == 1))
        fresh = smash_amd.optimize.ann_auto_graph(n, 2, au.FIT_CONTROL, au.FIT_BOUNDS, "adam", 0.003, au.FIT_SEED)
        assert au.same_bits(fresh.weights(), z["weights_0"])
        assert [int(l.neurons) for l in fresh._dense()] == [21, 10, 4]
    check_fit(case, run)
    assert run["net"].history["loss_valid"] == []
    lo, hi = np.array(au.FIT_BOUNDS).T
    for i, k in enumerate(au.FIT_CONTROL):                         # the planes come back whole and inside the bounds
        assert np.all(run["planes"][k] >= lo[i]) and np.all(run["planes"][k] <= hi[i])


def test_early_stopping_keeps_the_best_weights():
    plain, early = au.fixture("fit_auto_adam_4"), au.fixture("fit_auto_adam_4_early")
    assert np.array_equal(plain["loss_train"], early["loss_train"]) and not np.array_equal(plain["weights"], early["weights"])
    a, b = run_fit("auto_adam_4"), run_fit("auto_adam_4_early")
    assert a["loss_train"] == b["loss_train"] and not np.array_equal(a["weights"], b["weights"])
