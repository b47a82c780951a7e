"""CPU: the optimiser of the uniform calibration (smash_amd/csrc/sx_sbs.cpp behind smashx_sbs_*, include/smashx_sbs.h) fed with the
costs of the plain-C oracle (oracle/pyoracle.run, bit-identical to the reference) against the reference's own optimize_sbs, recorded
after k = 0 .. K iterations in tests/golden/sbs/ (tests/golden/make_sbs.py).  Equality is of fp32 bit patterns: the loop is the same
statement, there is no tolerance.  nfg is compared with the recorder's restatement, which reproduced the reference's costs and values
bit for bit when the fixture was written (the reference only prints nfg, and the recorded runs are silent)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import golden_util as gu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_sbs as ms  # noqa: E402

f32 = np.float32
FULL = ("gr_b_16x16x96_nse_gaps", "gr_a_12x12x48_nse")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    return _lib, _lib.lib()


def _load(name):
    return np.load(os.path.join(gu.GOLDEN_DIR, "sbs", name + ".npz"))


def drive(L, lower, upper, x0, cost0, maxiter, cost_of):
    """the ask / tell loop: per k = iter / n the (gx, x, nfg, ddx), then the message, iter, nfg and the final point"""
    from smash_amd import _lib
    n = len(x0)
    lower, upper, x0 = (np.ascontiguousarray(a, f32) for a in (lower, upper, x0))
    h = C.c_void_p()
    _lib.check(L.smashx_sbs_create(n, lower.ctypes.data, upper.ctypes.data, x0.ctypes.data, C.c_float(float(cost0)), maxiter, C.byref(h)))
    try:
        y, m, x = np.zeros((n, 2 * n), f32, order="F"), C.c_int(0), x0.copy()
        rows, done, batches = [(f32(cost0), x0.copy(), 1, f32(0.64))], 0, []
        while True:
            _lib.check(L.smashx_sbs_ask(h, y.ctypes.data, C.byref(m)))
            if m.value == 0:
                break
            assert 1 <= m.value <= 2 * n
            batches.append(m.value)
            f = np.array([cost_of(y[:, c].copy()) for c in range(m.value)], f32)
            _lib.check(L.smashx_sbs_tell(h, f.ctypes.data))
            it = L.smashx_sbs_iter(h)
            if it != done and it % n == 0:
                _lib.check(L.smashx_sbs_x(h, x.ctypes.data))
                rows.append((f32(L.smashx_sbs_gx(h)), x.copy(), int(L.smashx_sbs_nfg(h)), f32(L.smashx_sbs_ddx(h))))
            done = it
        _lib.check(L.smashx_sbs_x(h, x.ctypes.data))
        assert L.smashx_sbs_ask(h, y.ctypes.data, C.byref(m)) == 0 and m.value == 0          # finished stays finished
        return rows, L.smashx_sbs_message(h).decode(), int(L.smashx_sbs_iter(h)), int(L.smashx_sbs_nfg(h)), (f32(L.smashx_sbs_gx(h)), x.copy()), batches
    finally:
        L.smashx_sbs_destroy(h)


def _problem(z):
    from oracle import pyoracle
    fx = dict(case=str(z["case"]), fields=tuple(str(k) for k in z["fields"]), lb=tuple(z["lb"]), ub=tuple(z["ub"]), x0=tuple(z["x0"]), K=int(z["K"]))
    g, P, S, order, opts = ms.problem(fx)
    assert list(order) == list(fx["fields"])
    inner = ms.cost_function(g, P, S, order, opts, pyoracle.run)
    seen = {}

    def cost_of(y):          # the restatement and the library ask for the same points: evaluate each once
        key = np.asarray(y, f32).tobytes()
        if key not in seen:
            seen[key] = f32(inner(np.asarray(y, f32)))
        return seen[key]
    return fx, cost_of


@pytest.fixture(scope="module", params=sorted(ms.FIXTURES))
def run(request):
    _, L = _lib()
    z = _load(request.param)
    fx, cost_of = _problem(z)
    cost0 = cost_of(np.array(fx["x0"], f32))
    got = drive(L, fx["lb"], fx["ub"], fx["x0"], cost0, fx["K"], cost_of)
    return request.param, z, fx, cost_of, cost0, got


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_cost_and_point_after_every_iteration_equal_the_reference(run):
    name, z, fx, cost_of, cost0, (rows, msg, it, nfg, last, batches) = run
    n, K = len(fx["x0"]), fx["K"]
    assert _bits(cost0) == _bits(z["cost"][0]) and np.array_equal(_bits(fx["x0"]), _bits(z["x"][0]))
    for k in range(1, K + 1):
        # a run of maxiter = k ends at iterate k, or earlier at the point where DDX < 0.01 stopped it
        gx, x = (rows[k][0], rows[k][1]) if k * n <= it and k < len(rows) else last
        assert _bits(gx) == _bits(z["cost"][k]), (name, k, gx, z["cost"][k])
        assert np.array_equal(_bits(x), _bits(z["x"][k])), (name, k, x, z["x"][k])
        assert _bits(cost_of(x)) == _bits(gx)                 # what the final forward at x returns
    assert msg == str(z["task"]) and it == int(z["inner_iterations"])
    assert [r[2] for r in rows] == list(z["nfg"]) and nfg == int(z["nfg_total"])
    assert np.array_equal(_bits([r[3] for r in rows]), _bits(z["ddx"]))
    assert nfg == 1 + sum(batches)


def test_equals_the_recorders_restatement(run):
    """the numpy float32 restatement of tests/golden/make_sbs.py, a second statement of the loop: same trajectory, same count"""
    name, z, fx, cost_of, cost0, (rows, msg, it, nfg, last, batches) = run
    r_rows, r_msg, events, r_last = ms.sbs_restated(cost_of, fx["x0"], fx["lb"], fx["ub"], fx["K"], cost0)
    assert r_msg == msg and r_last[3] == it and r_last[2] == nfg and len(r_rows) == len(rows)
    for a, b in zip(rows, r_rows):
        assert _bits(a[0]) == _bits(b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2] and _bits(a[3]) == _bits(b[3])
    assert _bits(last[0]) == _bits(r_last[0]) and np.array_equal(_bits(last[1]), _bits(r_last[1]))
    assert sorted(events) == sorted(str(e) for e in z["events"])


def test_fixtures_meet_the_recorders_conditions():
    for name in FULL:
        z = _load(name)
        assert set(ms.ALL) <= set(str(e) for e in z["events"]), name
        fields = [str(k) for k in z["fields"]]
        lb, ub = z["lb"], z["ub"]
        kinds = {"asinh" if lo < 0 else "logit" if hi <= 1 else "log" for lo, hi in zip(lb, ub)}
        assert kinds == {"asinh", "logit", "log"} and "exc" in fields and "hp" in fields, (name, fields)
    assert str(_load("gr_a_12x12x48_nse_ddx")["task"]) == "CONVERGENCE: DDX < 0.01"
    assert str(_load("gr_b_16x16x96_nse_gaps_maxiter")["task"]) == "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT"
    for name in ms.FIXTURES:
        assert os.path.getsize(os.path.join(gu.GOLDEN_DIR, "sbs", name + ".npz")) < 64 * 1024


def test_ties_and_nan_never_win_and_the_first_of_equals_does():
    _, L = _lib()
    told = []

    def flat(y):
        told.append(y.copy())
        return f32(1.0)
    rows, msg, it, nfg, last, batches = drive(L, [1.0, -3.0], [100.0, 3.0], [10.0, 0.5], 1.0, 3, flat)
    assert _bits(last[0]) == _bits(f32(1.0)) and np.array_equal(_bits(last[1]), _bits(np.array([10.0, 0.5], f32)))       # an equal cost is no descent
    assert msg == "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT" and it == 6 and batches[0] == 4
    rows, msg, it, nfg, last, batches = drive(L, [1.0, -3.0], [100.0, 3.0], [10.0, 0.5], 1.0, 2, lambda y: f32(np.nan))
    assert _bits(last[0]) == _bits(f32(1.0)) and np.array_equal(_bits(last[1]), _bits(np.array([10.0, 0.5], f32)))
    # two candidates with the same lower cost: the first in (i, j) order is taken, the next iteration does not go back on it
    first = []

    def two_equal(y):
        first.append(y.copy())
        return f32(0.5) if len(first) in (1, 3) else f32(1.0)
    rows, msg, it, nfg, last, batches = drive(L, [1.0, -3.0], [100.0, 3.0], [10.0, 0.5], 1.0, 1, two_equal)
    assert np.array_equal(_bits(rows[1][1]), _bits(first[0])) and batches[:2] == [4, 3]


def test_maxiter_zero_runs_nothing():
    _, L = _lib()
    rows, msg, it, nfg, last, batches = drive(L, [1.0], [100.0], [10.0], 2.0, 0, lambda y: f32(0.0))
    assert msg == "" and it == 0 and nfg == 1 and batches == [] and _bits(last[0]) == _bits(f32(2.0))


def test_argument_checks():
    lib, L = _lib()
    one, h, m = np.array([1.0], f32), C.c_void_p(), C.c_int(0)
    lo, up = np.array([0.5], f32), np.array([2.0], f32)
    ok = (1, lo.ctypes.data, up.ctypes.data, one.ctypes.data, C.c_float(1.0), 5, C.byref(h))
    for i, bad in ((0, 0), (1, None), (2, None), (3, None), (5, -1), (6, None)):
        a = list(ok)
        a[i] = bad
        assert L.smashx_sbs_create(*a) == lib.E_ARG, i
    assert L.smashx_sbs_create(1, up.ctypes.data, lo.ctypes.data, one.ctypes.data, C.c_float(1.0), 5, C.byref(h)) == lib.E_ARG      # lower > upper
    assert L.smashx_sbs_create(*ok) == 0
    y = np.zeros((1, 2), f32, order="F")
    assert L.smashx_sbs_ask(None, y.ctypes.data, C.byref(m)) == lib.E_ARG and L.smashx_sbs_ask(h, None, C.byref(m)) == lib.E_ARG
    assert L.smashx_sbs_ask(h, y.ctypes.data, None) == lib.E_ARG
    assert L.smashx_sbs_tell(h, one.ctypes.data) == lib.E_STATE          # nothing asked
    assert L.smashx_sbs_ask(h, y.ctypes.data, C.byref(m)) == 0 and m.value == 2
    assert L.smashx_sbs_ask(h, y.ctypes.data, C.byref(m)) == lib.E_STATE          # a batch is open
    assert L.smashx_sbs_tell(h, None) == lib.E_ARG and L.smashx_sbs_tell(None, one.ctypes.data) == lib.E_ARG
    assert L.smashx_sbs_x(h, None) == lib.E_ARG and L.smashx_sbs_x(None, one.ctypes.data) == lib.E_ARG
    assert L.smashx_sbs_tell(h, np.array([3.0, 4.0], f32).ctypes.data) == 0
    assert L.smashx_sbs_iter(h) == 1 and L.smashx_sbs_nfg(h) == 3 and L.smashx_sbs_message(h) == b""
    assert L.smashx_sbs_iter(None) == 0 and L.smashx_sbs_nfg(None) == 0 and L.smashx_sbs_message(None) == b""
    assert L.smashx_sbs_destroy(h) == 0 and L.smashx_sbs_destroy(None) == 0
    # smashx_uniform_costs: what is refused before a plan is looked at
    rc = np.full(2, 123.0, f32)
    assert L.smashx_uniform_costs(None, None, None, 0, None, None, 2, rc.ctypes.data) == lib.E_ARG and np.all(rc == f32(123.0))
    assert L.smashx_uniform_costs_info(None, None, None) == lib.E_ARG


def test_optimize_sbs_is_exported_and_rejects_an_empty_control_vector():
    import smash_amd
    from smash_amd import synth
    assert callable(smash_amd.optimize_sbs) and callable(smash_amd.uniform_costs)
    m = synth.make_mesh(6, 6, ng=1)
    setup = smash_amd.SetupDT(0, 1, structure="gr-a", dt=3600.0, ntime_step=4)
    setup.optimize.optim_parameters = np.zeros(16, np.int32)
    setup.optimize.optim_states = np.zeros(8, np.int32)
    mesh = smash_amd.MeshDT.from_synth(setup, m)
    inp = smash_amd.Input_DataDT(setup, mesh)
    par = smash_amd.ParametersDT.from_dict(mesh, synth.make_parameters(6, 6))
    sta = smash_amd.StatesDT.from_dict(mesh, synth.make_states(6, 6))
    with pytest.raises(ValueError, match="nothing to optimise"):
        smash_amd.optimize_sbs(setup, mesh, inp, par, sta, smash_amd.OutputDT(setup, mesh))
    with pytest.raises(ValueError, match="candidates"):
        smash_amd.optimize_sbs(setup, mesh, inp, par, sta, smash_amd.OutputDT(setup, mesh), candidates="gpu")


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
SBS_HEADER = os.path.join(ROOT, "include", "smashx_sbs.h")


def test_sbs_header_matches_the_binding():
    """include/smashx_sbs.h against _lib.SBS_PROTOTYPES with the parser and the type rules tests/test_abi_header_cpu.py applies to
    smashx.h and PROTOTYPES; counts taken from the header's own text, so that a declaration the parser skips fails here"""
    import test_abi_header_cpu as ah
    from smash_amd import _lib
    text = open(SBS_HEADER).read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    assert [k for k in h["constants"] if k != "SMASHX_SBS_H"] == []
    assert re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", ah.strip(text)[0], flags=re.M) == ["SMASHX_SBS_H"]
    assert re.findall(r"\btypedef\b[^;]*;", ah.strip(text)[1]) == ["typedef struct smashx_sbs smashx_sbs;"]         # the one opaque handle
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == 12
    assert sorted(h["functions"]) == sorted(_lib.SBS_PROTOTYPES) and _lib.SBS_SYMBOLS == list(_lib.SBS_PROTOTYPES)
    others = [_lib.PROTOTYPES, _lib.SETUP_PROTOTYPES, _lib.FORCING_PROTOTYPES, _lib.PRCP_PROTOTYPES, _lib.SIGNATURE_PROTOTYPES,
              _lib.HYPER_DEVICE_PROTOTYPES, _lib.ANN_PROTOTYPES]
    assert not any(set(_lib.SBS_PROTOTYPES) & set(o) for o in others)
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.SBS_PROTOTYPES[name]
        if rptr:
            assert rbase == "char" and restype is C.c_char_p, name
        else:
            assert restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert list(h["functions"]) == list(_lib.SBS_PROTOTYPES)          # the header's order


def test_smashx_h_brings_the_sbs_header_along():
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    assert hdr.count('#include "smashx_sbs.h"') == 1
    assert hdr.index('#include "smashx_ann.h"') < hdr.index('#include "smashx_sbs.h"')
    assert "#define SMASHX_ABI_VERSION 9" in hdr


def test_symbols_are_exported_and_bound():
    lib, L = _lib()
    for name, (restype, argtypes) in lib.SBS_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.smashx_abi_sizes(None) == 9
