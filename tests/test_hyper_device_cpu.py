"""CPU: the device form of the hyper maps (include/smashx_hyper.h) as far as it goes without a GPU -- the header against the binding,
the exported symbols, the argument checks of the Python layer -- and smash_amd.optimize_hyper_lbfgsb, the mirror of
mw_optimize::optimize_hyper_lbfgsb (mw_optimize.f90:779-1177), against tests/golden/hyper_optimize/ (the compiled reference,
tests/golden/make_hyper_optimize.py): its problem initialisation exactly, and its loop, driven through the injectable evaluation by the
CPU oracle and the host maps of sx_hyper.cpp, to the bars tests/test_gpu_parity.py::test_optimize_lbfgsb_python_host uses."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import hyper_device_util as hu  # noqa: E402
from oracle import pyoracle  # noqa: E402

HYPER_HEADER = os.path.join(ROOT, "include", "smashx_hyper.h")
NAMES = ["smashx_hyper_set_descriptors", "smashx_hyper_upload", "smashx_hyper_gradient", "smashx_hyper_fields", "smashx_hyper_info"]


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_hyper_header_matches_the_binding():
    """include/smashx_hyper.h against _lib.HYPER_DEVICE_PROTOTYPES with the parser and the type rules tests/test_abi_header_cpu.py
    applies to smashx.h and PROTOTYPES; counts taken from the header's own text, so that a declaration the parser skips fails here"""
    import test_abi_header_cpu as ah
    from smash_amd import _lib
    text = open(HYPER_HEADER).read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    assert [k for k in h["constants"] if k != "SMASHX_HYPER_H"] == []
    assert re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", ah.strip(text)[0], flags=re.M) == ["SMASHX_HYPER_H"]
    assert not re.search(r"\b(struct|enum|typedef)\b", ah.strip(text)[1])
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == len(NAMES)
    assert list(h["functions"]) == NAMES == list(_lib.HYPER_DEVICE_PROTOTYPES) == _lib.HYPER_DEVICE_SYMBOLS
    others = (set(_lib.PROTOTYPES) | set(_lib.SETUP_PROTOTYPES) | set(_lib.FORCING_PROTOTYPES) | set(_lib.PRCP_PROTOTYPES)
              | set(_lib.SIGNATURE_PROTOTYPES))
    assert not set(_lib.HYPER_DEVICE_PROTOTYPES) & others
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.HYPER_DEVICE_PROTOTYPES[name]
        assert not rptr and restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert [p[:3] for p in h["functions"]["smashx_hyper_set_descriptors"][1]] == [
        ("plan", "smashx_plan", True), ("mapping", "int", False), ("nd", "int", False), ("descriptor", "float", True)]
    assert [p[:3] for p in h["functions"]["smashx_hyper_fields"][1]] == [
        ("plan", "smashx_plan", True), ("params", "smashx_parameters", True), ("states", "smashx_states", True)]
    # the comparison bites: a parameter turned into a pointer is reported
    flat = ah.parse(text.replace("int mapping, int nd,", "int mapping, int* nd,"))
    ah.check_type("nd", _lib.HYPER_DEVICE_PROTOTYPES["smashx_hyper_set_descriptors"][1][2],
                  *flat["functions"]["smashx_hyper_set_descriptors"][1][2][1:], flat, _lib, findings, param=True)
    assert findings and "nd" in findings[0]


def test_smashx_h_brings_the_hyper_header_along():
    """a C caller that includes smashx.h sees the declarations, after the signature header; no struct changed, so the ABI version stays"""
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    assert hdr.count('#include "smashx_hyper.h"') == 1
    assert hdr.index('#include "smashx_signature.h"') < hdr.index('#include "smashx_hyper.h"')
    assert "#define SMASHX_ABI_VERSION 9" in hdr


def test_symbols_are_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        restype, argtypes = _lib.HYPER_DEVICE_PROTOTYPES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.smashx_abi_sizes(None) == 9
    # the argument checks that need no plan
    assert L.smashx_hyper_set_descriptors(None, 1, 0, None) == _lib.E_ARG
    assert L.smashx_hyper_upload(None, None, None) == _lib.E_ARG
    assert L.smashx_hyper_gradient(None, None, None) == _lib.E_ARG
    assert L.smashx_hyper_fields(None, None, None) == _lib.E_ARG
    assert L.smashx_hyper_info(None, None, None) == _lib.E_ARG


# ---- argument checks of the Python layer ------------------------------------------------------------------------------------------------------
def test_descriptor_checks():
    import smash_amd
    from smash_amd import _lib
    good = np.zeros((5, 4, 2), np.float32, order="F")
    assert smash_amd.check_hyper_descriptors(5, 4, "hyper-linear", good) == (1, 2, good)
    assert smash_amd.check_hyper_descriptors(5, 4, "hyper-polynomial", np.zeros((5, 4, 0), np.float32, order="F"))[:2] == (2, 0)
    assert smash_amd.check_hyper_descriptors(5, 4, "hyper-polynomial", None) == (2, 1, None)
    for mapping, d in (("uniform", good), ("hyper-linear", good.astype(np.float64)), ("hyper-linear", np.ascontiguousarray(good)),
                       ("hyper-linear", np.zeros((4, 5, 2), np.float32, order="F")), ("hyper-linear", good[:, :, 0]),
                       ("hyper-linear", good.tolist())):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.check_hyper_descriptors(5, 4, mapping, d)
        assert e.value.code == _lib.E_ARG


def test_matrix_checks():
    import smash_amd
    from smash_amd import _lib
    hp, hs = np.zeros((3, 16), np.float32, order="F"), np.zeros((3, 8), np.float32, order="F")
    assert smash_amd.check_hyper_matrices(3, hp, hs) == (hp, hs)
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.check_hyper_matrices(None, hp, hs)
    assert e.value.code == _lib.E_STATE
    ro = hp.copy(order="F")
    ro.flags.writeable = False
    assert smash_amd.check_hyper_matrices(3, ro, hs)[0] is ro
    for a, b, w in ((hp[:2], hs, False), (hp, hs[:, :7], False), (hp.astype(np.float64), hs, False), (np.ascontiguousarray(hp), hs, False),
                    (hp, None, False), (hp.T, hs, False), (ro, hs, True)):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.check_hyper_matrices(3, a, b, writeable=w)
        assert e.value.code == _lib.E_ARG


# ---- the calibration ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", hu.MAPPINGS)
def test_problem_initialisation_equals_the_reference(mapping):
    """problem_initialise_hyper_lbfgsb + var_to_control_hyper_lbfgsb: x0, l, u and nbd of the compiled reference, exactly"""
    from smash_amd.optimize import hyper_problem_initialise
    g, z, setup, mesh, inp, par, sta, out = hu.calibration_case(mapping, 0)
    HP, HS, x0, l, u, nbd = hyper_problem_initialise(setup, mesh, par, sta)
    assert x0.dtype == np.float64 and np.array_equal(x0, z["x0"])
    assert np.array_equal(l, z["l"]) and np.array_equal(u, z["u"]) and np.array_equal(nbd, z["nbd"])
    nh = setup.optimize.nhyper
    assert x0.size == 4 * nh and np.count_nonzero(nbd) == (8 if mapping == "hyper-polynomial" else 0)
    # every field is mapped: the columns that are not flagged carry their inverse sigmoid too
    assert np.all(HP.matrix()[0] != 0) and np.all(HS.matrix()[0] != 0) and not HP.matrix()[1:, 0].any()


@pytest.fixture(scope="module")
def oracle_runs():
    """the loop over the CPU oracle, once per (mapping, maxiter): history, calibrated planes, input_data afterwards"""
    import smash_amd
    from smash_amd.solver import _hyper_to_fields
    runs = {}
    for mapping in hu.MAPPINGS:
        for it in (1, 4):
            g, z, setup, mesh, inp, par, sta, out = hu.calibration_case(mapping, it)
            seen = []

            def evaluate(hp, hs, setup=setup, mesh=mesh, inp=inp, g=g, seen=seen):
                HP, HS = smash_amd.Hyper_ParametersDT(setup), smash_amd.Hyper_StatesDT(setup)
                HP.set_matrix(hp)
                HS.set_matrix(hs)
                p, s = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
                _hyper_to_fields(setup, mesh, inp, p, HP, s, HS)
                seen.append((float(inp.descriptor.min()), float(inp.descriptor.max())))
                r = pyoracle.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, p.as_dict(), s.as_dict(), adjoint=True,
                                 jobs_fun=("nse",), wjobs_fun=(1.0,))
                hpb, hsb = hu.host_map_b(setup, mesh, inp, hp, hs, r["parameters_b"], r["states_b"])
                return r["cost"], hpb, hsb

            before = inp.descriptor.copy(order="F")
            h = smash_amd.optimize_hyper_lbfgsb(setup, mesh, inp, par, sta, out, evaluate=evaluate)
            runs[mapping, it] = dict(h=h, z=z, par=par, inp=inp, before=before, seen=seen, setup=setup)
    return runs


@pytest.mark.parametrize("mapping", hu.MAPPINGS)
def test_loop_over_the_oracle_follows_the_reference(oracle_runs, mapping):
    """after 1 iteration 3e-7 + 1e-5 |ref|, after 4 within 0.02 |ref[0]| (tests/test_gpu_parity.py:348-349); the first evaluation -- the
    maps and the sweep at x0, no optimiser yet -- to the first bar as well"""
    one, four = oracle_runs[mapping, 1], oracle_runs[mapping, 4]
    z = one["z"]
    ref = {int(m): float(z[f"cost_{int(m)}"]) for m in z["maxiters"]}
    print(mapping, "costs", one["h"]["cost_initial"], one["h"]["final_cost"], four["h"]["cost"], four["h"]["final_cost"],
          "reference", list(z["iter_costs_4"]), ref)
    ref0 = float(z["iter_costs_4"][0])
    assert abs(one["h"]["cost_initial"] - ref0) <= 3e-7 + 1e-5 * abs(ref0)
    assert len(one["h"]["cost"]) == 1 and len(four["h"]["cost"]) == 4
    assert abs(one["h"]["final_cost"] - ref[1]) <= 3e-7 + 1e-5 * abs(ref[1]), (one["h"]["final_cost"], ref)
    assert abs(four["h"]["final_cost"] - ref[4]) <= 0.02 * abs(ref[0]), (four["h"]["final_cost"], ref)
    assert four["h"]["final_cost"] < one["h"]["final_cost"] < one["h"]["cost_initial"]


@pytest.mark.parametrize("mapping", hu.MAPPINGS)
def test_loop_leaves_the_callers_objects_as_the_reference_does(oracle_runs, mapping):
    r = oracle_runs[mapping, 4]
    o = r["setup"].optimize
    # the evaluations saw descriptors normalised to [0, 1] over the whole grid; afterwards they are the caller's again
    assert all(lo == 0.0 and hi == 1.0 for lo, hi in r["seen"])
    assert hu.same_bits(r["inp"].descriptor, r["before"])
    assert np.array_equal(r["z"]["descriptor_norm"].min(axis=(0, 1)), [0, 0]) and np.array_equal(r["z"]["descriptor_norm"].max(axis=(0, 1)), [1, 1])
    # calibrated planes: mapped over the whole grid, inside the bounds, and they moved
    cp = r["par"].cp
    assert np.all(cp > o.lb_parameters[1]) and np.all(cp < o.ub_parameters[1]) and cp.std() > 0
    h = r["h"]
    assert h["hyper_parameters"].shape == (o.nhyper, 16) and h["hyper_states"].shape == (o.nhyper, 8)
    for k in ("cost", "nfg", "task", "final_cost", "cost_initial", "x0", "l", "u", "nbd"):
        assert k in h
    if mapping == "hyper-polynomial":           # the exponents stay in their box
        e = h["hyper_parameters"][2::2, np.flatnonzero(o.optim_parameters)]
        assert np.all(e >= 0.5) and np.all(e <= 2.0)
    # (not asserted: how close the matrices after one iteration are to the reference's own -- DESIGN.md 9g notes it)
    one = oracle_runs[mapping, 1]
    print(mapping, "max |hyper_parameters - reference| after one iteration", float(np.max(np.abs(one["h"]["hyper_parameters"] - one["z"]["hyper_parameters_1"]))),
          "cost bits equal:", hu.same_bits(np.float32(one["h"]["final_cost"]), one["z"]["cost_1"]))
