"""GPU: the routing kernels on the constructed river trees of tests/river_cases.py against the CPU oracle -- serpentine chains (a
group as deep as it is large, more steps and fewer steps than a group is deep, step counts around the 256-step publication period of
the chained launches), a comb (an inlet and a cell as the two children of every stem cell), chains of fans (seven children at interior
cells, most of them inlets at groups of 64, all in the group at 512; under every rotation; with holes in the D8 order and a ragged
mask), a forest of them under vic-a and gr-d, eight children at roots, and basins of one cell.  tests/test_river_cases_cpu.py holds
the meshes, their schedules and the oracle itself (against the compiled reference) on the CPU.

  a. The sweep (forward, adjoint, tangent along 1 % of cp, cft, lr) against the oracle by the rules of
     tests/test_gpu_parity_at_size.py (_check, imported): the exact-libm build BIT-IDENTICAL to the fp32 oracle on every forward and
     adjoint output -- what catches a wrong order of the children's sum --, the default build e_hip <= 2 e_ref + 1e-6 against the fp64
     oracle, costs <= 2 |ref - truth| + 3e-7, the tangent by the default rule in both builds.  e_ref is 1e-9 ... 5e-4 on these
     cases except on the outputs tests/test_river_cases_cpu.py pins as ill-conditioned (gr-b's ci_b and hi_b above all), where the
     default-build bar is a sanity bar.  Not vacuous: rounds, groups and deepest stage of the plan are the CPU schedule's; the cases
     with chained rounds ran them in one launch; nothing stalled.
  b. Switches that move addresses and launches only -- staging rows, launch per round, the circular routing tape, storage chunks
     of 16 and 32 steps (4 and 8 tape rows against groups 63 and 511 deep) with and without pipeline sub-chunks (the kept chain tape
     off and on), every group size -- on S1, S2, F1 and C1: every output bit-identical to the single-chunk default.
  c. The ensemble kernels (130 samples) and the resident kernel (5 samples) against the loop of forwards that (a) has just held to
     the oracle on the same meshes, bit for bit; a catchment the resident kernel cannot hold is refused in words.
  d. The same file under SMASHX_EXACT_LIBM=1 in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import multiple_run_util as mu
import river_cases as rc
from test_gpu_ensemble import _ensemble, _loop, _ndiff, _same
from test_gpu_parity_at_size import _check, _sweeps
from test_gpu_uniform_costs import _refused, _resident

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHAINED = ("S1", "S2", "S3-nt255", "S3-nt256", "S3-nt257", "S3-nt516", "F1")      # (and more: these are asserted)
_default = {}


def _swept(cid):
    """(outputs, plan) of case cid at its group size with the plan's defaults: one sweep per case, shared, left unchanged."""
    if cid not in _default:
        g = rc.build(cid)
        hip, plan = _sweeps(g, group_size=g.group)
        for v in hip.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _default[cid] = (hip, plan)
    return _default[cid]


def _plan_is_the_cpu_schedule(cid, plan):
    c = rc.CASES[cid]
    rounds, groups, _, deepest = rc.PLAN[(c["mesh"], c["group"])]
    assert (plan["n_rounds"], plan["n_groups"], plan["max_stage"]) == (rounds, groups, deepest), (cid, plan)


# ---- a. the sweep against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(rc.CASES))
def test_sweep_vs_oracle(cid, capfd):
    ref = rc.reference(cid)
    hip, plan = _swept(cid)
    bad = _check(cid, hip, ref)
    out, err = capfd.readouterr()
    with capfd.disabled():
        sys.stdout.write(out)
        sys.stderr.write(err)
    _plan_is_the_cpu_schedule(cid, plan)
    assert plan["n_chunks"] == 1, plan
    if cid in CHAINED:
        assert plan["n_chained_groups"] > 0 and plan["route_fwd_launches"] == 2, plan       # round 0 + one chained launch
    assert "stalled" not in err, err
    assert all(np.all(np.isfinite(np.asarray(v))) for v in hip.values())
    assert not bad, (cid, bad)


# ---- b. address-only switches --------------------------------------------------------------------------------------------------------
def _chunks(chunk, pipe, **env):
    return dict(env=env, kw=dict(chunk_steps=chunk, pipe_steps=pipe))


SWITCHES = {
    "stage0": dict(env=dict(SMASHX_CHAIN_STAGE="0")),
    "stage1": dict(env=dict(SMASHX_CHAIN_STAGE="1")),
    "launch-per-round": dict(env=dict(SMASHX_CHAIN_ROUNDS="0")),
    "skew0": dict(env=dict(SMASHX_HR_SKEW="0")),
    "skew1": dict(env=dict(SMASHX_HR_SKEW="1")),
    "chunk16": _chunks(16, 0),
    "chunk16-pipe16": _chunks(16, 16),
    "chunk32": _chunks(32, 0),
    "chunk32-pipe16": _chunks(32, 16),
    "chunk16-skew0": _chunks(16, 0, SMASHX_HR_SKEW="0"),
    "chunk16-stage1": _chunks(16, 0, SMASHX_CHAIN_STAGE="1"),
    "chunk32-pipe16-stage1": _chunks(32, 16, SMASHX_CHAIN_STAGE="1"),
    "chunk16-no-kept-tape": _chunks(16, 0, SMASHX_KEEP_CHAIN_TAPE="0"),
    "group64": dict(kw=dict(group_size=64)),
    "group128": dict(kw=dict(group_size=128)),
    "group256": dict(kw=dict(group_size=256)),
    "group512": dict(kw=dict(group_size=512)),
}
ENV = ("SMASHX_CHAIN_STAGE", "SMASHX_CHAIN_ROUNDS", "SMASHX_HR_SKEW", "SMASHX_KEEP_CHAIN_TAPE", "SMASHX_CHAIN_FROM")


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("cid", ["S1", "S2", "F1", "C1"])
def test_address_only_switches_are_bit_identical(cid, switch, monkeypatch, capfd):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    base, base_plan = _swept(cid)
    assert base_plan["n_chunks"] == 1 and base_plan["n_chained_groups"] > 0, base_plan
    g = rc.build(cid)
    sw = SWITCHES[switch]
    env, kw = sw.get("env", {}), dict({"group_size": g.group}, **sw.get("kw", {}))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    hip, plan = _sweeps(g, **kw)
    out, err = capfd.readouterr()
    with capfd.disabled():
        sys.stdout.write(f"{cid} {switch}: " + out)
        sys.stderr.write(err)
    assert "stalled" not in err, err
    # not vacuous: the switch took
    chained = plan["n_chained_groups"] > 0
    if "SMASHX_CHAIN_STAGE" in env:
        assert chained and plan["chain_staged"] == int(env["SMASHX_CHAIN_STAGE"]), plan
    if "SMASHX_CHAIN_ROUNDS" in env:
        assert not chained and plan["route_fwd_launches"] == plan["n_rounds"], plan
    if "chunk_steps" in kw:
        C = -(-g.nt // kw["chunk_steps"])
        assert plan["chunk_steps"] == kw["chunk_steps"] and plan["n_chunks"] == C and chained, plan
        assert (plan["pipe_steps"] < plan["chunk_steps"]) == (0 < kw["pipe_steps"] < kw["chunk_steps"]), plan
        if kw["pipe_steps"] == 0:       # the kept tape: the recomputed chunks run no chained forward launch
            kept = env.get("SMASHX_KEEP_CHAIN_TAPE", "1") == "1"
            assert plan["route_fwd_chained_launches"] == (C if kept else 2 * C - 1), plan
    if "group_size" in sw.get("kw", {}):
        c = rc.CASES[cid]
        if (c["mesh"], kw["group_size"]) in rc.PLAN:
            rounds, groups, _, deepest = rc.PLAN[(c["mesh"], kw["group_size"])]
            assert (plan["n_rounds"], plan["n_groups"], plan["max_stage"]) == (rounds, groups, deepest), plan
    assert set(hip) == set(base)
    differ = [k for k in base if not np.array_equal(np.asarray(hip[k]), np.asarray(base[k]))]
    assert not differ, (cid, switch, differ)


# ---- c. the other routers ------------------------------------------------------------------------------------------------------------
ROUTERS = ["S1", "C1", "F1", "F3-drop25", "F4-vic-a", "F4-gr-d", "E1"]
_loops = {}


def _loop_of(cid):
    """the ensemble's and the loop's costs and discharges of the 130 samples of a case, on one plan: computed once, shared"""
    if cid not in _loops:
        g = rc.build(cid)
        names = mu.fields_of(g.structure)
        sample = mu.draw(names, 130)
        ec, eq, ctx = _ensemble(g, names, sample, group_size=g.group)
        lc, lq = _loop(ctx, g, names, sample)
        for a in (ec, eq, lc, lq, sample):
            a.setflags(write=False)
        _loops[cid] = (g, names, sample, ctx, ec, eq, lc, lq)
    return _loops[cid]


@pytest.mark.parametrize("cid", ROUTERS)
def test_ensemble_equals_the_loop_bit_for_bit(cid):
    g, names, sample, ctx, ec, eq, lc, lq = _loop_of(cid)
    _plan_is_the_cpu_schedule(cid, ctx[2]._smashx_solver.timing())
    print(f"{cid}: 130 samples, costs differing {_ndiff(ec, lc)}, qsim values differing {_ndiff(eq, lq)}, finite costs {int(np.isfinite(lc).sum())}")
    assert np.any(np.isfinite(lc))
    assert _same(eq, lq)
    assert _same(ec, lc)


@pytest.mark.parametrize("cid", ROUTERS)
def test_resident_kernel_equals_the_loop_bit_for_bit(cid):
    g, names, sample, ctx, ec, eq, lc, lq = _loop_of(cid)
    s5 = np.asfortranarray(sample[:, :5])
    rcost = _resident(ctx, names, s5)
    info = ctx[2]._smashx_solver.uniform_costs_info()
    print(f"{cid}: {info}, loop {lc[:5]}, resident {rcost}")
    assert info["cells"] == g.mesh.nac and info["levels"] == rc.SHAPE[rc.CASES[cid]["mesh"]][2] + 1
    assert np.any(np.isfinite(lc[:5])) or g.structure == "vic-a"      # (vic-a blows up over much of the default bounds)
    assert _same(rcost, lc[:5])


def test_resident_kernel_refuses_the_long_snake_in_words():
    """S2 has 1320 cells, the resident kernel holds 1024: refused, not skipped, and the caller's array left alone"""
    from test_gpu_parity import _types
    g = rc.build("S2")
    names = ("cp", "lr")
    _refused(_types(g), names, mu.draw(names, 2), "1320 active cells")


# ---- d. the exact-libm build ---------------------------------------------------------------------------------------------------------
N_TESTS = len(rc.CASES) + 4 * len(SWITCHES) + 2 * len(ROUTERS) + 1


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=1500, cwd=ROOT)
    sys.stdout.write(r.stdout[-20000:])
    assert "exact: bit-identical" in r.stdout and "e_hip" in r.stdout       # (the tangent keeps the default rule)
    assert r.returncode == 0 and f"{N_TESTS} passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
