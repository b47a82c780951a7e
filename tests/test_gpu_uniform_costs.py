"""GPU: the catchment-resident cost route (smash_amd.uniform_costs -> smashx_uniform_costs, kernel in smash_amd/csrc/sx_resident.h)
against the loop of single forward runs it replaces, against the reference, at its limits and at the sizes where the time skew of its
levels can go wrong.  Every case runs in the build the session selects; test_exact_build_runs_this_file re-runs the file under
SMASHX_EXACT_LIBM=1.

"Bit for bit" as in tests/test_gpu_ensemble.py: equal fp32 bit patterns wherever either side is a number, a NaN at the same place on
both sides.  The samples are drawn inside the calibration box (tests/multiple_run_util.py)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import golden_util as gu
import multiple_run_util as mu
from test_gpu_ensemble import _loop, _same
from test_gpu_parity import _types

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S_MAX = 65
S_CASES = (1, 3, 9, 65)
DROW = (-1, -1, 0, 1, 1, 1, 0, -1)       # D8 codes 1..8 = N, NE, E, SE, S, SW, W, NW
DCOL = (0, 1, 1, 1, 0, -1, -1, -1)


def _resident(ctx, names, sample):
    import smash_amd
    setup, mesh, inp, par, sta, out = ctx
    return smash_amd.uniform_costs(setup, mesh, inp, par, sta, np.asfortranarray(sample), mu.index_of(names))


_loop_costs = {}


def _loop_of(key, g, names):
    """the loop's costs of the S_MAX samples of a case, computed once and shared (the first columns of a draw do not depend on S)"""
    if key not in _loop_costs:
        ctx = _types(g)
        sample = mu.draw(names, S_MAX)
        lc, _ = _loop(ctx, g, names, sample)
        lc.setflags(write=False)
        _loop_costs[key] = (ctx, sample, lc)
    return _loop_costs[key]


LOOP_CASES = ["gr_a_12x12x48_nse", "gr_b_16x16x96_nse_gaps", "gr_c_16x16x96_kge_se_log_mask", "gr_d_12x12x48_rmse_kge2_start",
              "vic_a_16x16x96_nse_gaps", "gr_a_16x16x96_median3", "gr_b_16x16x96_median2"]


@pytest.mark.parametrize("S", S_CASES)
@pytest.mark.parametrize("name", LOOP_CASES)
def test_equals_the_loop_bit_for_bit(name, S):
    g = gu.load(name)
    names = mu.fields_of(g.structure)
    ctx, sample, lc = _loop_of(name, g, names)
    rc = _resident(ctx, names, sample[:, :S])
    info = ctx[2]._smashx_solver.uniform_costs_info()
    print(f"{name} S={S}: {info}, costs differing {int(np.count_nonzero(rc.view(np.uint32) != lc[:S].view(np.uint32)))}")
    assert rc.shape == (S,) and _same(rc, lc[:S])


@pytest.mark.parametrize("names", [("lr", "hlr"), ("cp", "cft", "hp")], ids=["routing_side_only", "no_routing_side_field"])
def test_equals_the_loop_partial_sampling(names):
    """only lr and hlr sampled: every other field is the cell's own (distributed) value; and the converse"""
    g = gu.load("gr_c_16x16x96_kge_se_log_mask")
    ctx, sample, lc = _loop_of(("partial",) + names, g, names)
    for S in (3, 65):
        assert _same(_resident(ctx, names, sample[:, :S]), lc[:S])


def test_a_second_batch_equals_the_ensemble_bit_for_bit():
    """16384 + 3 samples: one more than a batch holds, so that both routes stage, launch and copy out a second, short batch.  The
    loop of single runs is not run at this count: include/smashx_sbs.h states res_cost to be smashx_multiple_run's, bit for bit."""
    import smash_amd
    g = gu.load("gr_a_12x12x48_nse")
    names = ("cp", "lr")
    S = 16384 + 3
    sample = mu.draw(names, S)
    ctx = _types(g)
    setup, mesh, inp, par, sta, out = ctx
    ec = np.zeros(S, np.float32)
    smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, mu.index_of(names), ec, np.zeros(0, np.float32))
    ens = inp._smashx_solver.multiple_run_info()
    rc = _resident(ctx, names, sample)
    print(f"S={S}: ensemble {ens}, resident {inp._smashx_solver.uniform_costs_info()}, "
          f"costs differing {int(np.count_nonzero(rc.view(np.uint32) != ec.view(np.uint32)))}")
    assert ens["n_batches"] == 2, ens
    assert rc.shape == (S,) and np.all(np.isfinite(ec)) and _same(rc, ec)


# ---- hand-made meshes --------------------------------------------------------------------------------------------------------------------
def _hand(flwdir, gauges, nt, structure="gr-b", dx=1000.0):
    """a case on a hand-made D8 plane: cells with a code in 0..8 are active (0: an outlet that points nowhere), -99 elsewhere"""
    from smash_amd import synth
    flwdir = np.asarray(flwdir, np.int32)
    nrow, ncol = flwdir.shape
    active = (flwdir >= 0).astype(np.int32)
    acc = np.where(active == 1, 0, -99).astype(np.int32)
    for r in range(nrow):
        for c in range(ncol):
            rr, cc = r, c
            while 0 <= rr < nrow and 0 <= cc < ncol and active[rr, cc] == 1:        # every cell counts on its whole path down
                acc[rr, cc] += 1
                d = flwdir[rr, cc]
                if d < 1:
                    break
                rr, cc = rr + DROW[d - 1], cc + DCOL[d - 1]
    g = types.SimpleNamespace()
    g.structure, g.dt, g.nt = structure, 3600.0, nt
    area = np.array([float(acc[r, c]) * dx * dx for r, c in gauges], np.float32)
    g.mesh = synth.Mesh(nrow, ncol, dx, np.where(active == 1, flwdir, -99), acc, synth.make_path(acc), active, gauges, area)
    g.prcp, g.pet = synth.dense_forcing(g.mesh, nt)
    t = np.arange(nt, dtype=np.float64)
    g.qobs = np.asfortranarray(np.stack([0.6 + 0.4 * np.sin(t / 7.0 + i) for i in range(len(gauges))]).astype(np.float32))
    g.params, g.states = synth.make_parameters(nrow, ncol), synth.make_states(nrow, ncol, warm=True)
    g.opts = {}
    return g


def _channel(n):
    return np.array([[3] * n, [-99] * n]), [(0, n - 1), (0, 0)]


def _comb(n):
    """a main stem of n cells flowing east in row 1; headwaters in row 0 drain south into stem cells 3, 7 and the LAST one, whose
    delay line is nlevels - 1 long; gauges at the outlet and on that headwater"""
    top = [-99] * n
    for c in (3, 7, n - 1):
        top[c] = 5
    return np.array([top, [3] * n]), [(1, n - 1), (0, n - 1)]


def _confluence8():
    return np.array([[4, 5, 6], [3, 0, 7], [2, 1, 8]]), [(1, 1), (0, 0)]


def _block(nactive):
    """5 x 13 cells draining east / south-east / south, the first 65 - nactive cells of row 0 (headwaters of the plane) masked"""
    from smash_amd import synth
    fd = np.array(synth.make_flwdir(5, 13))
    fd[0, :65 - nactive] = -99
    return fd, [(4, 12), (2, 6)]


HAND = {
    "single_cell": (lambda: (np.array([[-99, -99, -99], [-99, 5, -99], [-99, -99, -99]]), [(1, 1)]), 48),
    "channel_70_nt3": (lambda: _channel(70), 3),
    "channel_70_nt130": (lambda: _channel(70), 130),
    "comb_24": (lambda: _comb(24), 60),
    "confluence_of_eight": (_confluence8, 48),
    "cells_63": (lambda: _block(63), 48),
    "cells_64": (lambda: _block(64), 48),
    "cells_65": (lambda: _block(65), 48),
}


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_made_meshes_equal_the_loop(case):
    make, nt = HAND[case]
    fd, gauges = make()
    g = _hand(fd, gauges, nt)
    names = mu.fields_of(g.structure)
    ctx = _types(g)
    sample = mu.draw(names, 5)
    lc, _ = _loop(ctx, g, names, sample)
    rc = _resident(ctx, names, sample)
    info = ctx[2]._smashx_solver.uniform_costs_info()
    print(f"{case}: {info}, loop {lc}, resident {rc}")
    assert info["cells"] == int((fd >= 0).sum())
    if case.startswith("channel"):
        assert info["levels"] == 70 and (nt < info["levels"]) == (nt == 3)
    if case == "comb_24":
        assert info["levels"] == 24         # the stem's; the headwater above its last cell waits nlevels - 1 steps
    assert np.all(np.isfinite(lc)) and _same(rc, lc)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_equals_the_reference():
    """the 16 stored Cance samples: the exact build equals the reference's costs bit for bit, the default build is held to the bar
    tests/test_gpu_ensemble.py::test_equals_the_reference applies to the ensemble's costs"""
    from smash_amd import _lib
    g = gu.load("gr_a_cance_28x28x1440")
    names = mu.fields_of(g.structure)
    z = np.load(os.path.join(gu.GOLDEN_DIR, "multiple_run", "gr_a_cance_s16.npz"))
    sample = mu.draw(names, 130)[:, :16].copy(order="F")
    assert np.array_equal(z["sample"], sample) and np.array_equal(z["ind"], mu.index_of(names)), "the stored samples are not the test's"
    ctx = _types(g)
    rc = _resident(ctx, names, sample)
    c = z["res_cost"]
    print("cance, 16 samples:", ctx[2]._smashx_solver.uniform_costs_info(), "worst relative cost error",
          float(np.max(np.abs(rc.astype(np.float64) - c) / np.abs(c))), "exact build", _lib.EXACT)
    assert np.all(np.isfinite(c))
    if _lib.EXACT:
        assert _same(rc, c)
    else:
        for i in range(16):
            assert abs(float(rc[i]) - float(c[i])) <= gu.tol_cost(g.noise["cost"], float(c[i])), (i, rc[i], c[i])


# ---- limits and refusals ---------------------------------------------------------------------------------------------------------------
def _synthetic(nrow, ncol, nt=24):
    from smash_amd import synth
    g = types.SimpleNamespace()
    g.structure, g.dt, g.nt = "gr-b", 3600.0, nt
    g.mesh = synth.make_mesh(nrow, ncol, ng=2)
    g.prcp, g.pet = synth.dense_forcing(g.mesh, nt)
    t = np.arange(nt, dtype=np.float64)
    g.qobs = np.asfortranarray(np.stack([0.6 + 0.4 * np.sin(t / 7.0 + i) for i in range(2)]).astype(np.float32))
    g.params, g.states = synth.make_parameters(nrow, ncol), synth.make_states(nrow, ncol, warm=True)
    g.opts = {}
    return g


def test_1024_cells_are_accepted():
    g = _synthetic(32, 32)
    names = ("cp", "lr")
    ctx = _types(g)
    sample = mu.draw(names, 2)
    lc, _ = _loop(ctx, g, names, sample)
    rc = _resident(ctx, names, sample)
    info = ctx[2]._smashx_solver.uniform_costs_info()
    print(info)
    assert info["cells"] == 1024 and info["block"] == 1024 and _same(rc, lc)


def _refused(ctx, names, sample, word):
    import smash_amd
    from smash_amd import _lib
    setup, mesh, inp, par, sta, out = ctx
    rc = np.full(sample.shape[1], 123.0, np.float32)
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.uniform_costs(setup, mesh, inp, par, sta, sample, mu.index_of(names), rc)
    assert e.value.code == _lib.E_UNSUPPORTED and word in str(e.value), str(e.value)
    assert np.all(rc == np.float32(123.0))


def test_1025_cells_and_too_much_lds_are_refused():
    names = ("cp", "lr")
    sample = mu.draw(names, 2)
    _refused(_types(_synthetic(25, 41)), names, sample, "1025 active cells")
    # 512 headwaters, each draining into its own cell of a main stem of 512: delay lines of 1, 2, ... 512 steps
    fd = np.array([[5] * 512, [3] * 512])
    _refused(_types(_hand(fd, [(1, 511)], 4)), names, sample, "LDS")


def test_refusals_of_the_ensemble_hold_here():
    import smash_amd
    from smash_amd import _lib
    from smash_amd.solver import Solver
    g = gu.load("gr_b_16x16x96_nse_gaps")
    names = ("cp", "cft")
    sample = mu.draw(names, 4)
    ctx = _types(g)
    ctx[0].optimize.denormalize_forward = True
    _refused(ctx, names, sample, "denormalize_forward")
    ctx = _types(g)
    ctx[0].optimize.jreg_fun, ctx[0].optimize.wjreg_fun, ctx[0].optimize.wjreg = ["prior"], [1.0], 0.5
    _refused(ctx, names, sample, "wjreg")
    setup, mesh, inp, par, sta, out = _types(g)
    s = Solver(setup, mesh, owner_mask=np.ones((mesh.nrow, mesh.ncol), np.int32, order="F"), chunk_steps=96)      # one part that owns everything is still a tiled plan
    s.set_forcing(inp.prcp, inp.pet)
    rc = np.full(4, 123.0, np.float32)
    with pytest.raises(smash_amd.SmashxError) as e:
        s.uniform_costs(par, sta, sample, mu.index_of(names), res_cost=rc)
    assert e.value.code == _lib.E_UNSUPPORTED and "tiled" in str(e.value), str(e.value)
    assert np.all(rc == np.float32(123.0))
    s.close()
    # a signature criterion: the cost stage is the ensemble's, which does not hold them
    c = gu.load("gr_a_cance_28x28x1440")
    ctx = _types(c)
    ctx[0].optimize.jobs_fun, ctx[0].optimize.wjobs_fun = ["nse", "Crc"], [0.5, 0.5]
    ctx[2].mean_prcp = np.asfortranarray(np.load(os.path.join(gu.GOLDEN_DIR, "mean_forcing", "gr_a_cance_28x28x1440.npz"))["mean_prcp"])
    _refused(ctx, ("cp", "cft"), sample, "signature")
    # and the argument checks
    ctx = _types(g)
    setup, mesh, inp, par, sta, out = ctx
    for bad_ind, word in (([2, 2], "repeated"), ([2, 5], "not used"), ([2, 99], "outside")):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.uniform_costs(setup, mesh, inp, par, sta, sample, np.array(bad_ind, np.int32))
        assert e.value.code == _lib.E_ARG and word in str(e.value), str(e.value)


def test_leaves_the_plan_alone():
    import smash_amd
    g = gu.load("gr_b_16x16x96_nse_gaps")
    setup, mesh, inp, par, sta, out = _types(g)
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, 7)

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
    rc = smash_amd.uniform_costs(setup, mesh, inp, par, sta, sample, mu.index_of(names))
    assert inp._smashx_solver is solver
    assert out.cost == 123.0 and np.array_equal(out.qsim, qs0)
    for k in mu.FIELD_NAMES[:16]:
        assert id(getattr(par, k)) == ids[k] and _same(getattr(par, k), getattr(keep_p, k)), k
    for k in mu.FIELD_NAMES[16:]:
        assert _same(getattr(sta, k), getattr(keep_s, k)), k
    # the plan's gauge series and uploaded fields: a download without a sweep in between still gives the adjoint run's results
    o1 = smash_amd.OutputDT(setup, mesh)
    solver.download(False, None, None, o1)
    assert np.float32(o1.cost) == np.float32(o0.cost) and _same(o1.qsim, o0.qsim)
    o2, pb2, sb2 = adjoint()
    assert np.float32(o2.cost) == np.float32(o0.cost) and _same(o2.qsim, o0.qsim)
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert _same(getattr(pb2, k), getattr(pb0, k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert _same(getattr(sb2, k), getattr(sb0, k)), k
    assert rc.shape == (7,) and np.all(np.isfinite(rc))


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=1500, cwd=ROOT)
    sys.stdout.write(r.stdout[-8000:])
    assert r.returncode == 0 and "44 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
