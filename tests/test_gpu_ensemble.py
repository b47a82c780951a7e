"""GPU: the ensemble path (smash_amd.compute_multiple_run -> smashx_multiple_run, kernels in smash_amd/csrc/sx_ensemble.h) against
the loop of single forward runs it replaces, against the reference, and against its own batching.  Every case runs in the build
the session selects; test_exact_build_runs_this_file re-runs the file under SMASHX_EXACT_LIBM=1.

"Bit for bit" below: the fp32 bit patterns are equal wherever either side is a number (signed zeros and infinities included), and a
NaN stands at the same place on both sides.  The sign of a NaN is left out on purpose.  Samples drawn over the whole default bounds
blow up in vic-a (84 of the 130 samples of the case below end with a NaN cost, in the single run as well); from the step at which
a run has become NaN -- the same step on both sides -- the default build's loop gives 0xffc00000 where the ensemble gives 0x7fc00000
in 509 of 93 600 values.  IEEE 754 does not define the sign of a NaN result, and the wave-uniform shortcuts of sx_math.h choose
their path by what the 64 lanes of a wavefront hold: cells of one wild run in the loop, 64 different samples here.  Measured on an
MI355X: every other value, every cost and every NaN position identical; the exact-libm build identical in all 32 bits everywhere.
np.array_equal without equal_nan, read literally, cannot hold for an array that contains a NaN at all, not even against itself."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import golden_util as gu
import multiple_run_util as mu
from test_gpu_parity import _types

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S_LOOP = 130          # not a multiple of 64


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan]))


def _ndiff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.count_nonzero((_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))))


def _ensemble(g, names, sample, qsim=True, setup_edit=None, **kw):
    import smash_amd
    setup, mesh, inp, par, sta, out = _types(g, **kw)
    if setup_edit:
        setup_edit(setup)
    S = sample.shape[1]
    rc = np.zeros(S, np.float32)
    rq = np.zeros((mesh.ng, g.nt, S), np.float32, order="F") if qsim else np.zeros(0, np.float32)
    smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, mu.index_of(names), rc, rq)
    return rc, rq, (setup, mesh, inp, par, sta, out)


def _loop(ctx, g, names, sample):
    """S calls of smash_amd.forward with the fields filled by hand, on the same resident plan."""
    import smash_amd
    setup, mesh, inp, par, sta, out = ctx
    S = sample.shape[1]
    rc = np.zeros(S, np.float32)
    rq = np.zeros((mesh.ng, g.nt, S), np.float32, order="F")
    for i in range(S):
        p = smash_amd.ParametersDT.from_dict(mesh, mu.filled(par.as_dict(), names, sample[:, i]))
        s = smash_amd.StatesDT.from_dict(mesh, mu.filled(sta.as_dict(), names, sample[:, i]))
        o = smash_amd.OutputDT(setup, mesh)
        smash_amd.forward(setup, mesh, inp, p, p.copy(), s, s.copy(), o, np.float32(0))
        rc[i], rq[:, :, i] = np.float32(o.cost), o.qsim
    return rc, rq


LOOP_CASES = ["gr_a_cance_28x28x1440", "gr_b_16x16x96_nse_gaps", "gr_c_32x32x240_d8_ragged", "gr_d_12x12x48_rmse_kge2_start",
              "vic_a_24x24x240_d8_kge", "gr_b_16x16x96_median2"]


@pytest.mark.parametrize("name", LOOP_CASES)
def test_equals_the_loop_bit_for_bit(name):
    g = gu.load(name)
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, S_LOOP)
    rc, rq, ctx = _ensemble(g, names, sample)
    lc, lq = _loop(ctx, g, names, sample)
    print(f"{name}: {S_LOOP} samples, {len(names)} fields, costs differing {_ndiff(rc, lc)}, qsim values differing {_ndiff(rq, lq)}, "
          f"NaN sign only {int(np.count_nonzero(_bits(rq) != _bits(lq))) - _ndiff(rq, lq)}, finite costs {int(np.isfinite(lc).sum())}")
    assert _same(rq, lq)
    assert _same(rc, lc)


@pytest.mark.parametrize("names", [("lr", "hlr"), ("cp", "cft", "hp")], ids=["routing_side_only", "no_routing_side_field"])
def test_equals_the_loop_partial_sampling(names):
    """only lr and hlr sampled: the vertical part is identical across the lanes, the routing is not; and the converse"""
    g = gu.load("gr_c_32x32x240_d8_ragged")
    sample = mu.draw(names, S_LOOP)
    rc, rq, ctx = _ensemble(g, names, sample)
    lc, lq = _loop(ctx, g, names, sample)
    assert _same(rq, lq)
    assert _same(rc, lc)


@pytest.mark.parametrize("name", ["gr_a_cance_28x28x1440", "gr_b_16x16x96_nse_gaps"])
def test_equals_the_reference(name):
    from oracle import pyoracle, refbind
    from smash_amd import _lib
    g = gu.load(name)
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, S_LOOP)[:, :16].copy(order="F")
    rc, rq, _ = _ensemble(g, names, sample)
    refs = [("oracle", pyoracle.run)]
    if refbind.available():
        refs.append(("reference", refbind.run))
    stored = os.path.join(gu.GOLDEN_DIR, "multiple_run", "gr_a_cance_s16.npz")
    rows = []
    if name == "gr_a_cance_28x28x1440":
        z = np.load(stored)
        assert np.array_equal(z["sample"], sample) and np.array_equal(z["ind"], mu.index_of(names)), "the stored samples are not the test's"
        rows.append(("stored reference", z["res_cost"], z["res_qsim"]))
    for label, run in refs:
        c, q = np.zeros(16, np.float32), np.zeros_like(rq)
        for i in range(16):
            r = run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, mu.filled(g.params, names, sample[:, i]),
                    mu.filled(g.states, names, sample[:, i]), **g.opts)
            c[i], q[:, :, i] = r["cost"], r["qsim"]
        rows.append((label, c, q))
    assert all(np.all(np.isfinite(c)) for _, c, _ in rows)
    for label, c, q in rows:
        eq = max(gu.rel_l2(rq[k, :, i], q[k, :, i]) for k in range(g.mesh.ng) for i in range(16))
        ec = float(np.max(np.abs(rc.astype(np.float64) - c) / np.abs(c)))
        print(f"{name} vs {label}: worst rel-L2 of a discharge series {eq:.3e}, worst relative cost error {ec:.3e}, exact build {_lib.EXACT}")
    for label, c, q in rows:
        if _lib.EXACT:
            assert _same(rq, q), label
            assert _same(rc, c), label
        else:
            for i in range(16):
                for k in range(g.mesh.ng):
                    e = gu.rel_l2(rq[k, :, i], q[k, :, i])
                    assert e <= gu.tol(g.noise["qsim"][k]), (label, i, k, e)
                assert abs(float(rc[i]) - float(c[i])) <= gu.tol_cost(g.noise["cost"], float(c[i])), (label, i, rc[i], c[i])


def test_batches_and_chunks(monkeypatch):
    """SMASHX_ENS_BATCH / SMASHX_ENS_CHUNK (switch list) force a small batch and a short time chunk: same bits"""
    g = gu.load("gr_b_64x64x720_nse")
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, 200)
    rc, rq, ctx = _ensemble(g, names, sample)
    free = ctx[2]._smashx_solver.multiple_run_info()
    monkeypatch.setenv("SMASHX_ENS_BATCH", "64")
    monkeypatch.setenv("SMASHX_ENS_CHUNK", "100")
    fc, fq, ctx2 = _ensemble(g, names, sample)
    info = ctx2[2]._smashx_solver.multiple_run_info()
    print("unforced", free, "forced", info)
    assert info["batch"] == 64 and info["chunk"] == 100 and info["n_batches"] >= 4 and info["n_chunks"] >= 8, info
    assert free["n_batches"] == 1 and free["n_chunks"] == 1, free
    assert _same(fq, rq)
    assert _same(fc, rc)


def test_leaves_the_plan_alone():
    import smash_amd
    g = gu.load("gr_b_16x16x96_nse_gaps")
    setup, mesh, inp, par, sta, out = _types(g)
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, 70)

    def adjoint():
        p, s, o = par.copy(), sta.copy(), smash_amd.OutputDT(setup, mesh)
        pb, sb = par.copy(), sta.copy()
        smash_amd.forward_b(setup, mesh, inp, p, pb, p.copy(), p.copy(), s, sb, s.copy(), s.copy(), o, o.copy(), np.float32(0), np.float32(1))
        return o, pb, sb
    o0, pb0, sb0 = adjoint()
    solver = inp._smashx_solver
    keep_p, keep_s = par.copy(), sta.copy()
    ids = {k: id(getattr(par, k)) for k in mu.FIELD_NAMES[:16]}
    out.cost, qs0 = 123.0, out.qsim.copy()
    rc = np.zeros(70, np.float32)
    smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, mu.index_of(names), rc, np.zeros(0, np.float32))
    assert inp._smashx_solver is solver
    assert out.cost == 123.0 and np.array_equal(out.qsim, qs0)
    for k in mu.FIELD_NAMES[:16]:
        assert id(getattr(par, k)) == ids[k] and _same(getattr(par, k), getattr(keep_p, k)), k
    for k in mu.FIELD_NAMES[16:]:
        assert _same(getattr(sta, k), getattr(keep_s, k)), k
    o1, pb1, sb1 = adjoint()
    assert np.float32(o1.cost) == np.float32(o0.cost) and _same(o1.qsim, o0.qsim)
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert _same(getattr(pb1, k), getattr(pb0, k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert _same(getattr(sb1, k), getattr(sb0, k)), k
    assert np.all(np.isfinite(rc[np.isfinite(rc)])) and rc.shape == (70,)


def test_refusals_on_the_device_path():
    import smash_amd
    from smash_amd import _lib
    from smash_amd.solver import Solver
    g = gu.load("gr_b_16x16x96_nse_gaps")
    names = ("cp", "cft")
    sample = mu.draw(names, 4)

    def denorm(setup):
        setup.optimize.denormalize_forward = True

    def jreg(setup):
        setup.optimize.jreg_fun, setup.optimize.wjreg_fun, setup.optimize.wjreg = ["prior"], [1.0], 0.5
    for edit, word in ((denorm, "denormalize_forward"), (jreg, "wjreg")):
        with pytest.raises(smash_amd.SmashxError) as e:
            _ensemble(g, names, sample, setup_edit=edit)
        assert e.value.code == _lib.E_UNSUPPORTED and word in str(e.value), str(e.value)
    setup, mesh, inp, par, sta, out = _types(g)
    s = Solver(setup, mesh, owner_mask=np.ones((mesh.nrow, mesh.ncol), np.int32, order="F"), chunk_steps=96)      # one part that owns everything is still a tiled plan
    with pytest.raises(smash_amd.SmashxError) as e:
        s.multiple_run(par, sta, sample, mu.index_of(names))
    assert e.value.code == _lib.E_UNSUPPORTED and "tiled" in str(e.value), str(e.value)
    s.close()


def test_faster_than_the_loop_it_replaces():
    """Cance, S = 1024: median of 5 multiple_run calls against the median of 5 loops of S single smashx_forward calls on the same
    resident plan (wall clock, downloads included)."""
    import ctypes as C
    from smash_amd import _lib
    from smash_amd.solver import PARAM_NAMES, STATE_NAMES, _pack_const
    g = gu.load("gr_a_cance_28x28x1440")
    names = mu.fields_of(g.structure)
    S = 1024
    sample = mu.draw(names, S)
    setup, mesh, inp, par, sta, out = _types(g)
    rc = np.zeros(S, np.float32)
    import smash_amd
    smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, mu.index_of(names), rc, np.zeros(0, np.float32))   # warm-up
    s = inp._smashx_solver
    L = _lib.lib()

    def ensemble():
        t = time.perf_counter()
        s.multiple_run(par, sta, sample, mu.index_of(names), res_cost=rc)
        return time.perf_counter() - t
    te = sorted(ensemble() for _ in range(5))[2]
    info = s.multiple_run_info()
    p, st_ = par.copy(), sta.copy()
    P, k1 = _pack_const(p, PARAM_NAMES, _lib.Parameters)
    St, k2 = _pack_const(st_, STATE_NAMES, _lib.States)
    qs = np.zeros((mesh.ng, g.nt), np.float32, order="F")
    costs = _lib.Costs()
    lc = np.zeros(S, np.float32)

    def loop():
        t = time.perf_counter()
        for i in range(S):
            for k, v in zip(names, sample[:, i]):
                getattr(p if k in PARAM_NAMES else st_, k)[...] = v
            _lib.check(L.smashx_forward(s._h, C.byref(P), C.byref(P), C.byref(St), C.byref(St), qs.ctypes.data_as(C.c_void_p), C.byref(costs), None))
            lc[i] = costs.cost
        return time.perf_counter() - t
    loop()      # warm-up
    tl = sorted(loop() for _ in range(5))[2]
    print(f"cance S={S}: multiple_run {te * 1e3:.1f} ms (device {info['device_ms']:.1f} ms, batch {info['batch']}, chunk {info['chunk']}), "
          f"loop of {S} smashx_forward {tl * 1e3:.1f} ms, ratio {tl / te:.1f}")
    assert _same(rc, lc)
    assert te < tl


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=1500, cwd=ROOT)
    sys.stdout.write(r.stdout[-8000:])
    assert r.returncode == 0 and "14 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
