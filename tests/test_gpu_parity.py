"""GPU: the HIP path, called through the C ABI (smash_amd.forward / forward_b -> libsmashx.so), against
(1) the golden vectors produced by the unmodified reference Fortran and (2) the plain-C oracle.

Tolerance (BASELINE.json north_star: "within 1e-6 relative"): rel-L2 <= 1e-6
per gauge discharge series, per gradient field and per final-state field, cost within 1e-6 relative --
relaxed, output by output, to 3x the reference's OWN flag-to-flag noise where that is larger (golden_util.tol:
the reference built as its makefile does, -O3 + FMA, against the -O2 -ffp-contract=off parity build differs
by up to 1e-5 on gradient fields even on well-conditioned cases, and by 10-90 % on cold-start cases).
"""
import numpy as np
import pytest

import golden_util as gu
from smash_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _types(g, **solver_kw):
    import smash_amd
    setup = smash_amd.SetupDT(0, g.mesh.ng, structure=g.structure, dt=g.dt, ntime_step=g.nt)
    o = setup.optimize
    o.jobs_fun = list(g.opts.get("jobs_fun", ("nse",)))
    o.wjobs_fun = list(g.opts.get("wjobs_fun", (1.0,)))
    o.optimize_start_step = int(g.opts.get("optimize_start_step", 1))
    o.denormalize_forward = bool(g.opts.get("denormalize_forward", False))
    if "wgauge" in g.opts:
        o.wgauge = np.asarray(g.opts["wgauge"], np.float32)
    if "jreg_fun" in g.opts:
        o.jreg_fun, o.wjreg_fun, o.wjreg = list(g.opts["jreg_fun"]), list(g.opts["wjreg_fun"]), float(g.opts["wjreg"])
    if "optim_parameters" in g.opts:
        o.optim_parameters = np.asarray(g.opts["optim_parameters"], np.int32)
        o.optim_states = np.asarray(g.opts["optim_states"], np.int32)
    mesh = smash_amd.MeshDT.from_synth(setup, g.mesh)
    inp = smash_amd.Input_DataDT(setup, mesh)
    inp.prcp, inp.pet, inp.qobs = g.prcp, g.pet, g.qobs
    par = smash_amd.ParametersDT.from_dict(mesh, g.params)
    sta = smash_amd.StatesDT.from_dict(mesh, g.states)
    out = smash_amd.OutputDT(setup, mesh)
    inp._bgd = (smash_amd.ParametersDT.from_dict(mesh, g.opts["params_bgd"]), smash_amd.StatesDT.from_dict(mesh, g.opts["states_bgd"])) \
        if "params_bgd" in g.opts else (par.copy(), sta.copy())
    if solver_kw:
        from smash_amd.solver import Solver
        layout = solver_kw.pop("layout", None)       # compact forcing residency (tests/test_gpu_compact.py)
        s = Solver(setup, mesh, **solver_kw)
        if layout is not None:
            s.set_forcing_layout(**layout)
        s.set_forcing(inp.prcp, inp.pet)
        inp._smashx_solver = s
    return setup, mesh, inp, par, sta, out


def _run_forward(g, **kw):
    import smash_amd
    setup, mesh, inp, par, sta, out = _types(g, **kw)
    smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], out, np.float32(0))
    return par, sta, out


def _run_adjoint(g, **kw):
    import smash_amd
    setup, mesh, inp, par, sta, out = _types(g, **kw)
    par_b, sta_b = par.copy(), sta.copy()
    smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), out,
                        out.copy(), np.float32(0), np.float32(1))
    return par, sta, out, par_b, sta_b


ALL = gu.names()


@pytest.mark.parametrize("name", ALL)
def test_forward_vs_reference_golden(name):
    g = gu.load(name)
    par, sta, out = _run_forward(g)
    for i in range(g.mesh.ng):
        e = gu.rel_l2(out.qsim[i], g.fwd["qsim"][i])
        assert e <= gu.tol(g.noise["qsim"][i]), (i, e, g.noise["qsim"][i])
    assert abs(out.cost - g.fwd["cost"]) <= gu.tol_cost(g.noise["cost"], g.fwd["cost"]), (out.cost, g.fwd["cost"])
    # the regulariser is summed in the reference's order and passes through no libm: equal in both builds (sx_jreg.h)
    assert np.float32(out.cost_jreg).tobytes() == np.float32(g.fwd["cost_jreg"]).tobytes(), (out.cost_jreg, g.fwd["cost_jreg"])
    for k in gu.STRUCT_STATES[g.structure]:
        e = gu.rel_l2(getattr(out.fstates, k), g.fwd["fstates"][k])
        assert e <= gu.tol_fstate(k, g.noise["fstates"][k]), (k, e, g.noise["fstates"][k])
        assert np.array_equal(getattr(sta, k), g.fwd["states"][k]), k       # states are restored (forward.f90:72)


@pytest.mark.parametrize("name", ALL)
def test_adjoint_vs_reference_golden(name):
    g = gu.load(name)
    par, sta, out, par_b, sta_b = _run_adjoint(g)
    for i in range(g.mesh.ng):
        assert gu.rel_l2(out.qsim[i], g.adj["qsim"][i]) <= gu.tol(g.noise["qsim"][i])
    assert abs(out.cost - g.adj["cost"]) <= gu.tol_cost(g.noise["cost"], g.adj["cost"])
    report, bad = {}, {}
    for k in gu.STRUCT_PARAMS[g.structure]:
        report[k] = (gu.rel_l2(getattr(par_b, k), g.adj["parameters_b"][k]), gu.tol(g.noise["parameters_b"][k]))
    for k in gu.STRUCT_STATES[g.structure]:
        report[k] = (gu.rel_l2(getattr(sta_b, k), g.adj["states_b"][k]), gu.tol(g.noise["states_b"][k]))
    bad = {k: v for k, v in report.items() if not v[0] <= v[1]}
    assert not bad, report
    # fields the structure does not use come back zero, like parameters_b = 0 (forward_db.f90:10869) -- or, when
    # they are optimised under a regulariser, with the regulariser's gradient alone
    for k in synth.PARAM_NAMES:
        if k not in gu.STRUCT_PARAMS[g.structure]:
            assert np.array_equal(getattr(par_b, k), g.adj["parameters_b"][k]), k
    for k in synth.STATE_NAMES:
        if k not in gu.STRUCT_STATES[g.structure]:
            assert np.array_equal(getattr(sta_b, k), g.adj["states_b"][k]), k
    assert not np.any(par_b.beta)


@pytest.mark.parametrize("name", ["gr_b_16x16x96_nse_gaps", "gr_c_16x16x96_kge_se_log_mask", "gr_c_32x32x240_d8_ragged",
                                  "vic_a_24x24x240_d8_kge"])
@pytest.mark.parametrize("chunk,pipe,group", [(16, 0, 64), (32, 16, 128), (48, 32, 512), (0, 16, 256)])
def test_chunking_and_grouping_do_not_change_results(name, chunk, pipe, group):
    """Time-chunk checkpointing, the two-stream chunk pipeline and the routing partition only reorder
    independent work: results must be bit-identical to the single-chunk default."""
    g = gu.load(name)
    ref = _run_adjoint(g)
    alt = _run_adjoint(g, chunk_steps=chunk, pipe_steps=pipe, group_size=group)
    assert np.array_equal(ref[2].qsim, alt[2].qsim)
    assert ref[2].cost == alt[2].cost
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(ref[3], k), getattr(alt[3], k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(ref[4], k), getattr(alt[4], k)), k


def _staging_case(name, chunk, pipe, group, staged):
    """A parameter set of the staging test; its id stays name-chunk-pipe-group (staged is the plan's expected state, not a variant)."""
    return pytest.param(name, chunk, pipe, group, staged, id=f"{name}-{chunk}-{pipe}-{group}")


@pytest.mark.parametrize("name,chunk,pipe,group,staged", [_staging_case("gr_c_32x32x240_d8_ragged", 96, 16, 64, False),
                                                          _staging_case("gr_b_64x64x720_nse", 240, 48, 128, True),
                                                          _staging_case("vic_a_24x24x240_d8_kge", 64, 32, 64, False),
                                                          _staging_case("gr_b_20x20x96_d8", 0, 0, 64, False),
                                                          _staging_case("gr_b_64x64x720_nse", 0, 0, 512, False)])
def test_staging_rows_of_the_chained_groups_equal_the_plain_rows(name, chunk, pipe, group, staged, monkeypatch):
    """The chained routing launches read their inputs from -- and, in the reverse sweep, write their results to -- staging rows indexed
    by time block + stage, filled and emptied by the LDS-FIFO transposition passes (sx_k_chain_transpose, sx_kernels.h "Staging rows"):
    a change of addresses only.  Every output bit-identical with SMASHX_CHAIN_STAGE=0, across storage chunks, sub-chunks and group sizes.
    staged: the plan really runs on staging rows (chain_staged); the others have two routing rounds only, so no round is chained
    (chain_first needs two rounds after the first) and there is nothing to stage -- asserted, so that no case passes vacuously."""
    g = gu.load(name)
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", "0")
    ref = _run_adjoint(g, chunk_steps=chunk, pipe_steps=pipe, group_size=group)
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", "1")
    import smash_amd
    setup, mesh, inp, par, sta, out = _types(g, chunk_steps=chunk, pipe_steps=pipe, group_size=group)
    par_b, sta_b = par.copy(), sta.copy()
    smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), out,
                        out.copy(), np.float32(0), np.float32(1))
    alt = (par, sta, out, par_b, sta_b)
    tm = inp._smashx_solver.timing()
    if staged:
        assert tm["n_chained_groups"] > 0 and tm["chain_staged"] == 1, tm
    else:
        assert tm["n_chained_groups"] == 0 and tm["chain_staged"] == 0, tm
    assert np.array_equal(ref[2].qsim, alt[2].qsim) and ref[2].cost == alt[2].cost
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(ref[3], k), getattr(alt[3], k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(ref[4], k), getattr(alt[4], k)), k


@pytest.mark.parametrize("name,chunk,pipe", [("gr_b_20x20x96_d8", 0, 0), ("gr_c_32x32x240_d8_ragged", 48, 16), ("vic_a_24x24x240_d8_kge", 64, 32)])
def test_routing_tape_indexed_by_super_step_equals_rows_of_time_blocks(name, chunk, pipe, monkeypatch):
    """The hr_imd tape of the routing kernels is indexed by time block + the slot's stage (one row per super-step and group,
    DESIGN.md 8) unless the extra rows do not fit or SMASHX_HR_SKEW=0: an address change only -- every output bit-identical, also
    across storage chunks and pipeline sub-chunks (the shifted rows of consecutive launches interleave)."""
    g = gu.load(name)
    monkeypatch.setenv("SMASHX_HR_SKEW", "0")
    ref = _run_adjoint(g, chunk_steps=chunk, pipe_steps=pipe)
    monkeypatch.setenv("SMASHX_HR_SKEW", "1")
    alt = _run_adjoint(g, chunk_steps=chunk, pipe_steps=pipe)
    assert np.array_equal(ref[2].qsim, alt[2].qsim) and ref[2].cost == alt[2].cost
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(ref[3], k), getattr(alt[3], k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(ref[4], k), getattr(alt[4], k)), k


@pytest.mark.parametrize("name,chunk", [("gr_b_16x16x96_nse_gaps", 0), ("gr_c_16x16x96_kge_se_log_mask", 32), ("gr_b_24x24x120_norm_jreg", 48),
                                        ("gr_c_32x32x240_d8_ragged", 0)])
def test_interception_level_rebuilt_from_checkpoints_equals_tape(name, chunk, monkeypatch):
    """gr-b / gr-c: the reverse kernel either reads a tape of the interception level or rebuilds it block by block from
    sparse checkpoints (chosen by the plan when the full tape would force a second storage chunk; SMASHX_HI_TAPE forces it):
    the same sx_interception on the same operands, so every output is bit-identical -- also with gaps, with a step count
    that is not a multiple of the block (120, 240 vs 8) and across storage chunks."""
    g = gu.load(name)
    monkeypatch.setenv("SMASHX_HI_TAPE", "1")
    ref = _run_adjoint(g, chunk_steps=chunk)
    monkeypatch.setenv("SMASHX_HI_TAPE", "0")
    alt = _run_adjoint(g, chunk_steps=chunk)
    assert np.array_equal(ref[2].qsim, alt[2].qsim) and ref[2].cost == alt[2].cost
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(ref[3], k), getattr(alt[3], k)), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(ref[4], k), getattr(alt[4], k)), k


def test_sparse_forcing_layout_matches_dense():
    """Input_DataDT%sparse_prcp/pet (nac,nt) numbered along path (mw_sparse_storage.f90:12-49)."""
    import smash_amd
    g = gu.load("gr_c_16x16x96_kge_se_log_mask")
    _, _, dense = _run_forward(g)
    setup, mesh, inp, par, sta, out = _types(g)
    setup.sparse_storage = True
    act = g.mesh.active_cell
    idx = [(r, c) for r, c in zip(g.mesh.path[0], g.mesh.path[1]) if r >= 0 and c >= 0 and act[r, c] == 1]
    rr = np.array([i[0] for i in idx]); cc = np.array([i[1] for i in idx])
    inp2 = smash_amd.Input_DataDT(setup, mesh)
    inp2.sparse_prcp = np.asfortranarray(g.prcp[rr, cc, :]); inp2.sparse_pet = np.asfortranarray(g.pet[rr, cc, :])
    inp2.qobs = g.qobs
    smash_amd.forward(setup, mesh, inp2, par, par.copy(), sta, sta.copy(), out, np.float32(0))
    assert np.array_equal(out.qsim, dense.qsim)


def test_denormalize_forward_vs_oracle():
    """denormalize_forward path (forward.f90:33-38, DENORMALIZE_*_B forward_db.f90:967-1057,1959-2014),
    checked against the oracle on the normalised golden case with the regulariser switched off."""
    from oracle import pyoracle
    g = gu.load("gr_b_24x24x120_norm_jreg")
    opts = {k: v for k, v in g.opts.items() if k not in ("jreg_fun", "wjreg_fun", "wjreg")}
    g.opts = opts
    ref_f = pyoracle.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, **opts)
    ref_b = pyoracle.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, adjoint=True, **opts)
    par, sta, out = _run_forward(g)
    assert gu.rel_l2(out.qsim, ref_f["qsim"]) <= TOL and abs(out.cost - ref_f["cost"]) <= gu.tol_cost(g.noise["cost"], ref_f["cost"])
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(par, k), ref_f["parameters"][k]), k     # denormalised + round trip, exact affine ops
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(sta, k), ref_f["states"][k]), k
    par, sta, out, par_b, sta_b = _run_adjoint(g)
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert gu.rel_l2(getattr(par_b, k), ref_b["parameters_b"][k]) <= gu.tol(g.noise["parameters_b"][k]), k
        assert np.array_equal(getattr(par, k), ref_b["parameters"][k]), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert gu.rel_l2(getattr(sta_b, k), ref_b["states_b"][k]) <= gu.tol(g.noise["states_b"][k]), k


def test_unsupported_options_fail_loudly():
    import smash_amd
    g = gu.load("gr_a_24x24x120_norm_prior")
    setup, mesh, inp, par, sta, out = _types(g)
    setup.optimize.jreg_fun, setup.optimize.wjreg_fun, setup.optimize.wjreg = ["no_such_regulariser"], [1.0], 1e-2
    with pytest.raises(smash_amd.SmashxError):
        smash_amd.forward(setup, mesh, inp, par, par.copy(), sta, sta.copy(), out, np.float32(0))


def test_smoke_entry():
    import __graft_entry__
    __graft_entry__.smoke()


@pytest.mark.parametrize("blo,bhi", [(1.0, 2.0), (1.0, 4.0), (5.0, 7.0)])
def test_device_division_matches_ieee(blo, bhi):
    """sx_fdiv (6 instructions) against hipcc's IEEE a/b on the denominators the kernels feed it:
    1 + h*tanh in [1, 2], t + 2 in [1, 4], 6 - x*t near 6.  Never off by more than one ulp, and the
    one-ulp cases must be rarer than the ~1.5e-3 of calls where the correctly rounded powf already
    differs from glibc (tests/test_sx_math.py)."""
    import ctypes as C
    from smash_amd import _lib
    n = 200_000_000
    out = (C.c_longlong * 2)()
    fn = _lib.lib().smashx_selftest_math
    _lib.check(fn(0, n, 12345, blo, bhi, out))
    assert out[1] == 0
    assert out[0] <= n * 1e-6, (out[0], n)


def test_wavefront_fast_paths_equal_the_branchy_forms():
    """The straight-line paths a wavefront takes when all its lanes hold ordinary operands (sx_tanhf for |x| < ln2 / 4, the fp64
    log2 / pow of vic-a for positive normal bases) against the branchy restatements they shortcut, on the device, bit for bit --
    wavefronts of uniform small arguments (the path runs) and wavefronts mixed with large / special operands (it must not)."""
    import ctypes as C
    from smash_amd import _lib
    out = (C.c_longlong * 2)()
    fn = _lib.lib().smashx_selftest_paths
    for seed in (1, 777):
        _lib.check(fn(0, 100_000_000, seed, out))
        assert out[0] == 0 and out[1] == 0, list(out)


@pytest.mark.parametrize("name,sparse", [("gr_c_16x16x96_kge_se_log_mask", False), ("gr_b_16x16x96_nse_gaps", True)])
def test_domain_outputs(name, sparse):
    """setup%save_qsim_domain / save_net_prcp_domain (md_forward_structure.f90:158-194): discharge and net rainfall of
    every active cell and step, dense (-99 on inactive cells) or in the sparse (nac, nt) form; also across chunks."""
    import smash_amd
    from oracle import pyoracle
    from smash_amd.solver import Solver
    g = gu.load(name)
    ref = pyoracle.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, save_domain=True,
                       **{k: v for k, v in g.opts.items() if k in ("jobs_fun", "wjobs_fun", "optimize_start_step")})
    setup, mesh, inp, par, sta, out = _types(g)
    setup.save_qsim_domain = setup.save_net_prcp_domain = True
    act = g.mesh.active_cell
    if sparse:
        setup.sparse_storage = True
        idx = [(r, c) for r, c in zip(g.mesh.path[0], g.mesh.path[1]) if r >= 0 and c >= 0 and act[r, c] == 1]
        rr = np.array([i[0] for i in idx]); cc = np.array([i[1] for i in idx])
        inp = smash_amd.Input_DataDT(setup, mesh)
        inp.sparse_prcp = np.asfortranarray(g.prcp[rr, cc, :]); inp.sparse_pet = np.asfortranarray(g.pet[rr, cc, :])
        inp.qobs = g.qobs
    out = smash_amd.OutputDT(setup, mesh)
    s = Solver(setup, mesh, chunk_steps=32)
    if sparse:
        s.set_forcing(inp.sparse_prcp, inp.sparse_pet, sparse=True)
    else:
        s.set_forcing(inp.prcp, inp.pet)
    inp._smashx_solver = s
    smash_amd.forward(setup, mesh, inp, par, par.copy(), sta, sta.copy(), out, np.float32(0))
    qd = out.sparse_qsim_domain if sparse else out.qsim_domain
    pd = out.sparse_net_prcp_domain if sparse else out.net_prcp_domain
    if sparse:
        rq, rp = ref["qsim_domain"][rr, cc, :], ref["net_prcp_domain"][rr, cc, :]
    else:
        rq, rp = ref["qsim_domain"], ref["net_prcp_domain"]
        assert np.all(qd[act != 1] == -99.0) and np.all(pd[act != 1] == -99.0)
        for i in range(g.mesh.ng):      # the gauge cell of the domain array IS output%qsim
            assert np.array_equal(qd[g.mesh.gauge_pos[i, 0], g.mesh.gauge_pos[i, 1], :], out.qsim[i])
    # net rainfall of the data-gap steps is a difference of nearly equal powers (md_gr_operator.f90:94-96): 2e-6 there
    assert gu.rel_l2(qd, rq) <= 1e-6 and gu.rel_l2(pd, rp) <= 5e-6, (gu.rel_l2(qd, rq), gu.rel_l2(pd, rp))


def test_optimize_lbfgsb_python_host():
    """smash_amd.optimize_lbfgsb (host mirror of mw_optimize::optimize_lbfgsb over GPU sweeps) against the reference's own
    trajectory (tests/golden/lbfgsb, all-CPU): iteration-0 cost identical, same decrease after 4 iterations.  With the CPU
    oracle as the gradient provider this loop reproduces the reference's costs bit for bit (test_oracle_golden.py)."""
    import os
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "opt_gr_b_24x24x120.npz"))
    g = gu.load("gr_b_24x24x120_norm_jreg")
    g.opts = dict(jobs_fun=("nse",), wjobs_fun=(1.0,))
    g.params, g.states, g.qobs = synth.make_parameters(24, 24), synth.make_states(24, 24, warm=True), z["qobs"]
    costs = []
    for it in (1, 4):
        setup, mesh, inp, par, sta, out = _types(g)
        setup.optimize.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
        setup.optimize.maxiter = it
        h = smash_amd.optimize_lbfgsb(setup, mesh, inp, par, sta, out)
        costs.append(h["final_cost"])
        assert len(h["cost"]) == it
    ref = z["costs"]
    assert abs(costs[0] - ref[1]) <= 3e-7 + 1e-5 * abs(ref[1]), (costs, ref)
    assert abs(costs[1] - ref[4]) <= 0.02 * abs(ref[0]), (costs, ref)
    assert np.all(par.cp > 1.0)          # calibrated fields come back denormalised


def test_optimize_lbfgsb_with_adjusted_bounds_on_cance():
    """The reference's "adjust bounds" test (tests/core/test_simu.py:128-140): distributed L-BFGS-B over cp and cft on the Cance
    data with cp bounded to [1, 300], one iteration from the default parameters; cost and both calibrated fields against the
    reference's optimize_lbfgsb (tests/golden/lbfgsb/bounds_gr_a_cance.npz).  The bounds enter through the normalisation of the
    control (mwd_parameters_manipulation.f90:154-178), so a wrong bound moves every cell."""
    import os
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "bounds_gr_a_cance.npz"))
    g = gu.load("gr_a_cance_28x28x1440")
    g.params = {k: np.asfortranarray(np.full((g.mesh.nrow, g.mesh.ncol), synth.PARAM_DEFAULTS[k], np.float32)) for k in synth.PARAM_NAMES}
    setup, mesh, inp, par, sta, out = _types(g)
    o = setup.optimize
    o.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
    o.lb_parameters, o.ub_parameters = np.asarray(z["lb_parameters"], np.float32), np.asarray(z["ub_parameters"], np.float32)
    o.maxiter = int(z["maxiter"])
    h = smash_amd.optimize_lbfgsb(setup, mesh, inp, par, sta, out)
    assert abs(h["final_cost"] - float(z["cost"])) <= 1e-5 * abs(float(z["cost"])), (h["final_cost"], z["cost"])
    act = np.asarray(g.mesh.active_cell) == 1
    assert np.max(np.abs(par.cp[act] - z["final_cp"][act])) <= 1e-4 * 200.0, np.max(np.abs(par.cp[act] - z["final_cp"][act]))
    assert np.max(np.abs(par.cft[act] - z["final_cft"][act])) <= 1e-4 * 500.0
    assert np.ptp(par.cp[act]) > 0.5                    # the step really moved the field
    assert np.all(par.cp[act] <= 300.0) and np.all(par.cp[act] >= 1.0)


@pytest.mark.parametrize("start", ["defaults", "sbs"])
@pytest.mark.parametrize("mode", ["fast", "lcurve"])
def test_auto_wjreg_cycles_on_cance_vs_reference(mode, start):
    """The reference's own auto_wjreg test (tests/core/test_simu.py:143-170) on its own catchment: the real Cance data, control cp,
    cft, lr, prior + smoothing weighted 1 and 2, two iterations per cycle, 8 L-curve cycles -- from the model's default parameters
    and from the uniform SBS optimum (there two iterations remove < 5 % of the misfit: the L-curve tries nothing, chooses nothing and
    the model is left as it was).  Every cycle a smash_amd.optimize_lbfgsb over GPU sweeps, against the same cycles run by the
    reference's optimize_lbfgsb (tests/golden/lbfgsb/auto_wjreg_gr_a_cance*.npz)."""
    import os
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "auto_wjreg_gr_a_cance" + ("" if start == "defaults" else "_flat") + ".npz"))
    g = gu.load("gr_a_cance_28x28x1440")
    g.opts = dict(g.opts, jreg_fun=("prior", "smoothing"), wjreg_fun=(1.0, 2.0), wjreg=0.0)
    if start == "defaults":
        g.params = {k: np.asfortranarray(np.full((g.mesh.nrow, g.mesh.ncol), synth.PARAM_DEFAULTS[k], np.float32)) for k in synth.PARAM_NAMES}
    setup, mesh, inp, par, sta, out = _types(g)
    setup.optimize.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
    setup.optimize.maxiter = int(z["maxiter"])
    cp0 = par.cp.copy()
    h = smash_amd.optimize_lbfgsb(setup, mesh, inp, par, sta, out, auto_wjreg=mode, nb_wjreg_lcurve=int(z["nb_wjreg_lcurve"]),
                                  return_lcurve=True)
    rec = z[mode + "_cycles"]
    rel = lambda a, b: abs(a - b) / abs(b)
    if np.isnan(z[mode + "_wjreg"]):
        assert h["wjreg"] is None and h["lcurve"]["wjreg"].size == 1 and np.array_equal(par.cp, cp0)
        assert rel(h["lcurve"]["cost_jobs"][0], rec[0, 2]) <= 2e-4
        return
    assert rel(h["wjreg"], float(z[mode + "_wjreg"])) <= 1e-3, (h["wjreg"], z[mode + "_wjreg"])
    assert rel(out.cost, rec[-1, 1]) <= 5e-4 and rel(out.cost_jobs, rec[-1, 2]) <= 5e-4 and rel(out.cost_jreg, rec[-1, 3]) <= 2e-3, \
        (out.cost, out.cost_jobs, out.cost_jreg, rec[-1])
    assert gu.rel_l2(par.cp, z[mode + "_final_cp"]) <= 1e-4
    if mode == "lcurve":
        lc = h["lcurve"]
        assert lc["wjreg"].size == len(rec) - 1 and np.allclose(lc["wjreg"], rec[:-1, 0], rtol=1e-3)
        assert np.allclose(lc["cost_jobs"], rec[:-1, 2], rtol=5e-4) and np.allclose(lc["cost_jreg"], rec[:-1, 3], rtol=2e-3, atol=1e-9)
        assert np.array_equal(np.isnan(lc["distance"]), np.isnan(z["lcurve_distance"]))
        assert np.allclose(np.nan_to_num(lc["distance"]), np.nan_to_num(z["lcurve_distance"]), atol=2e-3)     # the values too (the costs differ by 5e-4)


@pytest.mark.parametrize("mode", ["fast", "lcurve"])
def test_auto_wjreg_cycles_vs_reference(mode):
    """SURVEY row f2, the weight of the regularisation term found by calibration cycles (auto_wjreg, core/simulation/
    _optimize.py:257-453; the reference's own test configuration, tests/core/test_simu.py:143-170: cp, cft, lr, prior + smoothing
    weighted 1 and 2, two iterations per cycle, 8 L-curve cycles): every cycle a smash_amd.optimize_lbfgsb over GPU sweeps, against
    the same cycles run by the reference's optimize_lbfgsb (tests/golden/lbfgsb/auto_wjreg_*.npz)."""
    import os
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "auto_wjreg_gr_b_24x24x120.npz"))
    g = gu.load("gr_b_24x24x120_norm_jreg")
    g.opts = dict(jobs_fun=("nse",), wjobs_fun=(1.0,), jreg_fun=("prior", "smoothing"), wjreg_fun=(1.0, 2.0), wjreg=0.0)
    g.params, g.states, g.qobs = synth.make_parameters(24, 24), synth.make_states(24, 24, warm=True), z["qobs"]
    setup, mesh, inp, par, sta, out = _types(g)
    setup.optimize.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
    setup.optimize.maxiter = int(z["maxiter"])
    h = smash_amd.optimize_lbfgsb(setup, mesh, inp, par, sta, out, auto_wjreg=mode, nb_wjreg_lcurve=int(z["nb_wjreg_lcurve"]),
                                  return_lcurve=True)
    rec = z[mode + "_cycles"]
    rel = lambda a, b: abs(a - b) / abs(b)
    assert rel(h["wjreg"], float(z[mode + "_wjreg"])) <= 2e-4, (h["wjreg"], z[mode + "_wjreg"])
    assert setup.optimize.wjreg == pytest.approx(h["wjreg"])
    assert rel(h["cost_jobs_initial"], float(z["cost_jobs_initial"])) <= 1e-5
    # the final cycle: cost, its two parts and the calibrated field
    assert rel(out.cost, rec[-1, 1]) <= 2e-4 and rel(out.cost_jobs, rec[-1, 2]) <= 2e-4 and rel(out.cost_jreg, rec[-1, 3]) <= 1e-3, \
        (out.cost, out.cost_jobs, out.cost_jreg, rec[-1])
    assert gu.rel_l2(par.cp, z[mode + "_final_cp"]) <= 1e-4
    if mode == "lcurve":
        lc = h["lcurve"]
        assert lc["wjreg"].size == len(rec) - 1
        assert np.allclose(lc["wjreg"], rec[:-1, 0], rtol=2e-4)
        assert np.allclose(lc["cost_jobs"], rec[:-1, 2], rtol=2e-4) and np.allclose(lc["cost_jreg"], rec[:-1, 3], rtol=1e-3)
        assert np.array_equal(np.isnan(lc["distance"]), np.isnan(z["lcurve_distance"]))
        assert np.allclose(np.nan_to_num(lc["distance"]), np.nan_to_num(z["lcurve_distance"]), atol=2e-4)


def test_optimize_lbfgsb_python_host_on_cance():
    """The same loop on the real Cance data (distributed calibration of the user guide, real_case_cance.rst:470-552)."""
    import os
    import smash_amd
    z = np.load(os.path.join(gu.GOLDEN_DIR, "lbfgsb", "opt_gr_a_cance.npz"))
    g = gu.load("gr_a_cance_28x28x1440")
    costs = []
    for it in (1, 6):
        setup, mesh, inp, par, sta, out = _types(g)
        setup.optimize.optim_parameters = np.asarray(z["optim_parameters"], np.int32)
        setup.optimize.maxiter = it
        h = smash_amd.optimize_lbfgsb(setup, mesh, inp, par, sta, out)
        costs.append(h["final_cost"])
    ref = z["costs"]
    assert abs(costs[0] - ref[1]) <= 3e-7 + 1e-5 * abs(ref[1]), (costs, ref)
    assert abs(costs[1] - ref[4]) <= 0.02 * abs(ref[0]), (costs, ref)


@pytest.mark.parametrize("case", ["nt5", "thin", "allgap", "one_cell", "no_gauge"])
def test_edge_cases_vs_oracle(case):
    """Ragged sizes the kernels' blocking must survive (steps not a multiple of 4, a 1-row grid, a single active cell),
    forcing that is one long data gap, and a plan without gauges: forward and adjoint against the oracle."""
    import smash_amd
    from oracle import pyoracle
    nrow, ncol, nt, ng = 9, 11, 23, 2
    if case == "nt5":
        nt = 5
    if case == "thin":
        nrow, ncol = 1, 37
    if case == "no_gauge":
        ng = 0
    m = synth.make_mesh(nrow, ncol, ng=max(ng, 1))
    if case == "one_cell":
        act = np.zeros((nrow, ncol), np.int32, order="F")
        r, c = int(m.gauge_pos[0, 0]), int(m.gauge_pos[0, 1])
        act[r, c] = 1
        fd = np.asfortranarray(np.where(act == 1, m.flwdir, -99).astype(np.int32))
        fa = synth.flow_accumulation(fd, act)
        m = synth.Mesh(nrow, ncol, m.dx, fd, fa, synth.make_path(np.where(act == 1, fa, -99)), act, m.gauge_pos[:1], m.area[:1] * 0 + m.dx * m.dx)
        ng = 1
    if case == "no_gauge":
        m = synth.Mesh(nrow, ncol, m.dx, m.flwdir, m.flwacc, m.path, m.active_cell, np.zeros((0, 2), np.int32), np.zeros(0, np.float32))
    prcp, pet = synth.dense_forcing(m, nt, gap_per_million=20000)
    if case == "allgap":
        prcp[...] = -99.0
    P, S = synth.make_parameters(nrow, ncol), synth.make_states(nrow, ncol, warm=True)
    qobs = np.asfortranarray(np.abs(np.random.default_rng(3).standard_normal((m.ng, nt))).astype(np.float32) + 0.1)
    g = type("G", (), {})()
    g.structure, g.dt, g.nt, g.mesh, g.prcp, g.pet, g.qobs, g.params, g.states, g.opts = "gr-c", 3600.0, nt, m, prcp, pet, qobs, P, S, {}
    _compare_with_oracle(g)


def _compare_with_oracle(g, bar=2e-5, plan=False):
    """Forward and adjoint of case g against the plain-C oracle (bit-identical to the reference): default build within `bar`; under the
    exact-libm build (tests/test_gpu_exact.py runs these tests with SMASHX_EXACT_LIBM=1) BIT-IDENTICAL -- cases without a golden vector
    have no reference noise to set a bar by, but the exact build must reproduce the oracle to the last bit: discharge, cost, final
    states and every gradient field."""
    from oracle import pyoracle
    from smash_amd import _lib
    m, st = g.mesh, g.structure
    fo = pyoracle.run(st, m, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
    bo = pyoracle.run(st, m, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, adjoint=True)
    par, sta, out = _run_forward(g)
    if plan:            # the adjoint through a Solver of its own, whose plan is returned (smashx_get_timing)
        import smash_amd
        setup, mesh, inp, par, sta, out2 = _types(g, chunk_steps=0)
        par_b, sta_b = par.copy(), sta.copy()
        smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), out2,
                            out2.copy(), np.float32(0), np.float32(1))
        tm = inp._smashx_solver.timing()
    else:
        par, sta, out2, par_b, sta_b = _run_adjoint(g)
        tm = None
    if _lib.EXACT:
        bad = []
        if m.ng:
            bad += [k for k, a, b in (("qsim", out.qsim, fo["qsim"]), ("cost", np.float32(out.cost), np.float32(fo["cost"])))
                    if not np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))]
        bad += ["fstates." + k for k in gu.STRUCT_STATES[st] if not np.array_equal(getattr(out.fstates, k), fo["fstates"][k])]
        bad += [k + "_b" for k in gu.STRUCT_PARAMS[st] if not np.array_equal(getattr(par_b, k), bo["parameters_b"][k])]
        bad += [k + "_b" for k in gu.STRUCT_STATES[st] if not np.array_equal(getattr(sta_b, k), bo["states_b"][k])]
        assert not bad, bad
        return tm
    if m.ng:
        assert gu.rel_l2(out.qsim, fo["qsim"]) <= 2e-6 and abs(out.cost - fo["cost"]) <= 1e-5 * abs(fo["cost"]) + 3e-7
    else:
        assert out.cost == 0.0
    for k in gu.STRUCT_STATES[st]:
        assert gu.rel_l2(getattr(out.fstates, k), fo["fstates"][k]) <= bar, k
    for k in gu.STRUCT_PARAMS[st]:
        assert gu.rel_l2(getattr(par_b, k), bo["parameters_b"][k]) <= bar, k
    for k in gu.STRUCT_STATES[st]:
        assert gu.rel_l2(getattr(sta_b, k), bo["states_b"][k]) <= bar, k
    return tm


@pytest.mark.parametrize("staged", [False, True])
def test_real_river_network_vs_oracle(staged, monkeypatch):
    """A REAL river network at size (VERDICT r3 missing 4): the largest basin of the reference's 1-km D8 raster of France
    (synth.make_mesh_france(1): 139 742 cells in a 535 x 399 box, all eight D8 codes, 6 routing rounds, the chained launch over 22 groups),
    gr-b, 96 steps, forward and adjoint against the oracle -- default build 2e-5, exact-libm build bit-identical.  staged: the chained
    launches on staging rows (what a plan with many chained groups does by itself, forced here: SMASHX_CHAIN_STAGE=1)."""
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", "1" if staged else "0")
    m = synth.make_mesh_france(1, ng=4)
    nt = 96
    prcp, pet = synth.dense_forcing(m, nt, gap_per_million=2000)
    P, S = synth.make_parameters(m.nrow, m.ncol), synth.make_states(m.nrow, m.ncol, warm=True)
    qobs = np.asfortranarray(np.abs(np.random.default_rng(5).standard_normal((m.ng, nt))).astype(np.float32) + 0.1)
    g = type("G", (), {})()
    g.structure, g.dt, g.nt, g.mesh, g.prcp, g.pet, g.qobs, g.params, g.states, g.opts = "gr-b", 3600.0, nt, m, prcp, pet, qobs, P, S, {}
    tm = _compare_with_oracle(g, plan=True)
    assert tm["n_chained_groups"] > 0 and tm["chain_staged"] == int(staged), tm       # the staged case really runs on staging rows


def test_error_behaviour():
    """The reference has no error channel; the C ABI returns a code + message and the Python host raises:
    a flow-direction cycle, a gauge outside the active domain, a signature-based criterion, a missing field."""
    import smash_amd
    from smash_amd import _lib
    g = gu.load("gr_a_12x12x48_nse")
    setup, mesh, inp, par, sta, out = _types(g)
    bad = smash_amd.MeshDT.from_synth(setup, g.mesh)
    fd = np.array(bad.flwdir, order="F")
    fd[5, 5], fd[5, 6] = 3, 7                       # E <-> W: a pit pair
    bad.flwdir = fd
    inp2 = smash_amd.Input_DataDT(setup, bad)
    inp2.prcp, inp2.pet, inp2.qobs = g.prcp, g.pet, g.qobs
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.forward(setup, bad, inp2, par, par.copy(), sta, sta.copy(), out, np.float32(0))
    assert e.value.code == _lib.E_MESH
    setup.optimize.jobs_fun = ["Crc"]
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.forward(setup, mesh, inp, par, par.copy(), sta, sta.copy(), out, np.float32(0))
    assert e.value.code == _lib.E_UNSUPPORTED
    setup.optimize.jobs_fun = ["nse"]
    bgd = par.copy()
    par.cp = None
    with pytest.raises(smash_amd.SmashxError) as e:
        smash_amd.forward(setup, mesh, inp, par, bgd, sta, sta.copy(), out, np.float32(0))
    assert e.value.code == _lib.E_ARG


def test_forcing_written_in_place_is_not_served_from_the_cache():
    """The plan (with the forcing resident in HBM) is cached on the input_data object.  Rain written IN PLACE into the same array
    -- what the f90wrap setters of the reference do -- must reach the device: the second run has to equal a fresh run on the
    new values, not the first run (the cache key used to be the array's address and shape)."""
    import smash_amd
    g = gu.load("gr_b_16x16x96_nse_gaps")
    setup, mesh, inp, par, sta, out = _types(g)
    smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    q1 = out.qsim.copy()
    s1 = inp._smashx_solver
    inp.prcp[:, :, 10:40] *= np.float32(1.5)                       # same array object, same address
    smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    q2 = out.qsim.copy()
    assert inp._smashx_solver is s1                                # the plan itself is kept, only the forcing went up again
    g2 = gu.load("gr_b_16x16x96_nse_gaps")
    g2.prcp = inp.prcp.copy(order="F")
    fresh = _run_forward(g2)[2].qsim
    assert not np.array_equal(q1, q2) and np.array_equal(q2, fresh)
    # explicit invalidation (for edits of a LARGE field that the sampled fingerprint could miss): the forcing goes up again
    fp = s1._fp
    smash_amd.invalidate_forcing(inp)
    assert s1._fp is None
    smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    assert inp._smashx_solver is s1 and s1._fp == fp and np.array_equal(out.qsim, q2)
    # a different mesh of the same shape (one more inactive cell) must rebuild the plan
    mesh.active_cell = np.asfortranarray(mesh.active_cell.copy())
    r, c = np.argwhere((np.asarray(mesh.flwacc) == 1) & (np.asarray(mesh.active_cell) == 1))[0]
    mesh.active_cell[r, c] = 0
    smash_amd.forward(setup, mesh, inp, par.copy(), inp._bgd[0], sta.copy(), inp._bgd[1], out, np.float32(0))
    assert inp._smashx_solver is not s1


@pytest.mark.parametrize("name", ["gr_b_24x24x120_norm_jreg", "gr_c_32x32x240_d8_ragged"])
def test_control_vector_on_the_device_equals_host_packing(name):
    """smashx_control_set / smashx_control_gradient (control_to_var_lbfgsb / var_to_control_lbfgsb, mw_optimize.f90:679-777, on the
    device) against the host path: fields scattered with numpy, uploaded, gradient fields downloaded and gathered.  Same cost, same
    discharge, same gradient vector to the bit -- with a regulariser, on a masked D8 mesh, flagged fields the structure does not use."""
    import smash_amd
    g = gu.load(name)
    g.opts = dict(g.opts)
    already = bool(g.opts.get("denormalize_forward", False))           # the *_norm_* fixtures hold normalised fields already
    g.opts["denormalize_forward"] = True
    op = np.zeros(16, np.int32); op[[1, 3, 4, 6, 15]] = 1              # cp, cft, cst (unused by gr-b), exc, lr
    os_ = np.zeros(8, np.int32); os_[[1, 7]] = 1                        # hp, hlr
    g.opts["optim_parameters"], g.opts["optim_states"] = op, os_
    setup, mesh, inp, par, sta, out = _types(g, chunk_steps=0)
    o = setup.optimize
    # the optimiser's space: normalised fields
    for names, obj, lb, ub in (() if already else ((synth.PARAM_NAMES, par, o.lb_parameters, o.ub_parameters), (synth.STATE_NAMES, sta, o.lb_states, o.ub_states))):
        for i, k in enumerate(names):
            setattr(obj, k, np.asfortranarray(((getattr(obj, k) - np.float32(lb[i])) / (np.float32(ub[i]) - np.float32(lb[i]))).astype(np.float32)))
    bgd_p, bgd_s = (par.copy(), sta.copy()) if "params_bgd" not in g.opts else inp._bgd
    sol = inp._smashx_solver
    if mesh.ng:
        sol.set_qobs(inp.qobs)
    sol.set_options(o)
    act = (np.asarray(mesh.active_cell) == 1).reshape(-1, order="F")
    m = int(act.sum())
    pf = [k for i, k in enumerate(synth.PARAM_NAMES) if op[i]]
    sf = [k for i, k in enumerate(synth.STATE_NAMES) if os_[i]]
    assert sol.control_size() == m * (len(pf) + len(sf))
    rng = np.random.default_rng(5)
    x = np.clip(np.concatenate([getattr(par, k).reshape(-1, order="F")[act] for k in pf] +
                               [getattr(sta, k).reshape(-1, order="F")[act] for k in sf]).astype(np.float64)
                + rng.normal(0, 0.01, m * (len(pf) + len(sf))), 0.0, 1.0)
    # host path
    p2, s2 = par.copy(), sta.copy()
    for j, k in enumerate(pf):
        a = getattr(p2, k).reshape(-1, order="F").copy(); a[act] = x[j * m:(j + 1) * m]
        setattr(p2, k, np.asfortranarray(a.reshape(mesh.nrow, mesh.ncol, order="F").astype(np.float32)))
    for j, k in enumerate(sf):
        a = getattr(s2, k).reshape(-1, order="F").copy(); a[act] = x[(len(pf) + j) * m:(len(pf) + j + 1) * m]
        setattr(s2, k, np.asfortranarray(a.reshape(mesh.nrow, mesh.ncol, order="F").astype(np.float32)))
    pb, sb = par.copy(), sta.copy()
    o1 = smash_amd.OutputDT(setup, mesh)
    sol.upload(p2, s2, bgd_p, bgd_s)
    sol.sweep(True, 1.0)
    sol.download(True, None, None, o1, pb, sb)
    g_host = np.concatenate([getattr(pb, k).reshape(-1, order="F")[act].astype(np.float64) for k in pf] +
                            [getattr(sb, k).reshape(-1, order="F")[act].astype(np.float64) for k in sf])
    # device path: the un-perturbed fields go up once, then only the control vector moves
    o2 = smash_amd.OutputDT(setup, mesh)
    sol.upload(par, sta, bgd_p, bgd_s)
    sol.control_set(x)
    sol.sweep(True, 1.0)
    sol.cost_and_qsim(o2)
    g_dev = sol.control_gradient()
    assert o1.cost == o2.cost and np.array_equal(o1.qsim, o2.qsim)
    assert np.array_equal(g_host, g_dev)
    # var_to_control of what the device holds: the normalise(denormalise(x)) round trip, x to fp32 accuracy (fields the structure
    # does not read come back from the regulariser's plane when there is one, else as zeros)
    xg = sol.control_get()
    for j, k in enumerate(pf + sf):
        used = k in gu.STRUCT_PARAMS[g.structure] or k in gu.STRUCT_STATES[g.structure]
        seg = xg[j * m:(j + 1) * m]
        if used or setup.optimize.jreg_fun:
            assert np.allclose(seg, x[j * m:(j + 1) * m].astype(np.float32), rtol=2e-6, atol=2e-7), k
        else:
            assert not seg.any(), k
