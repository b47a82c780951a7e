"""GPU: the sweep against the CPU oracle at the sizes the numbers are quoted at -- many cells (512^2, the 957 k-cell forest of
real basins of France, 384^2 vic-a and regularised gr-c) and the real horizon (8760 hourly steps, a year).  What only happens at
size is reached here and asserted from the plan (smashx_get_timing): chained routing launches over more groups than the device
holds at once, staging rows switched on by the plan's own rule (no SMASHX_CHAIN_STAGE), several storage chunks with a ragged last
chunk at 8760 steps, the compact forcing layout over a year, the median over many gauges, whole-grid regulariser sums.

Bars (fixed before the first run on the card, not tuned after it):
  * exact-libm build (SMASHX_EXACT_LIBM=1, run by tests/test_gpu_exact.py): BIT-IDENTICAL to the fp32 oracle on every forward and
    adjoint output -- discharge per gauge, cost, final states, every gradient field of the structure (_compare_with_oracle's rule).
    The tangent outputs are not held to bit-identity: no test holds the exact build's tangent to it today (the tangent sweep sums
    the cost derivative in its own order), so they take the default-build rule below in both builds.  What holds the tangent in
    both builds is tests/test_gpu_tangent_fields.py: every field's own direction against the fp64 truth and against the adjoint
    sweep of the same build.
  * default build: per output o, e_hip = rel_l2(hip, truth64) <= 2 e_ref + 1e-6 with e_ref = rel_l2(oracle32, truth64) -- the
    timed build is no farther from the exact answer than the reference is, within a factor 2.  truth64 = the same statements in
    double (oracle/liboracle64.so).  Costs: |hip - truth| <= 2 |ref - truth| + 3e-7 (the floor of golden_util.tol_cost).
    At 8760 steps the fp32 reference itself is 1e-6 .. 1e-1 away from the truth: a fixed bar would be unreachable
    or meaningless there.
Every output prints one line: e_hip, e_ref and rel_l2(hip, oracle32).  The oracle runs (fp32 and, in the default build, fp64) take
two to three minutes on 8 processes and are made once, up front (size_cases.oracle_all)."""
import time

import numpy as np
import pytest

import golden_util as gu
import size_cases as sc
from test_gpu_compact import SYNTH_LAYOUT
from test_gpu_parity import _types

pytestmark = pytest.mark.gpu

IDS = ("W1", "W3", "W4", "W5", "L1", "L2", "L3", "L4")
TANGENT = ("qsim_d", "cost_d")
SCALAR = ("cost", "adj.cost", "cost_d")
# outputs exempted from the default-build bar (name: reason with its fp64 evidence); none so far
EXEMPT = {}

_oracle = {}
_gpu_w1 = {}


def _exact():
    from smash_amd import _lib
    return _lib.EXACT


def _ref(cid):
    """(qobs, {False: oracle fp32 outputs, True: fp64 outputs}) of case cid; all cases at once on the first call."""
    if not _oracle:
        t = time.time()
        _oracle.update(sc.oracle_all(IDS, fp64=True, fp64_kinds=("tan",) if _exact() else ("fwd", "adj", "tan")))
        print(f"oracle stage: {time.time() - t:.0f} s wall")
    return _oracle[cid]


def _case(cid):
    q, ref = _ref(cid)
    return sc.build(cid, q), ref


def _sweeps(g, tangent=True, **kw):
    """Forward, adjoint and (where the case has a direction) tangent sweeps of case g through smash_amd.forward / forward_b /
    forward_d with Solver keyword arguments kw: flat dict of outputs (the keys of size_cases.oracle_outputs) and the plan's timing
    and forcing info after the adjoint sweep."""
    import smash_amd
    ps, ss = gu.STRUCT_PARAMS[g.structure], gu.STRUCT_STATES[g.structure]
    kw = dict({"chunk_steps": 0}, **kw)          # (a Solver of its own, so that its plan can be read)
    out = {}
    setup, mesh, inp, par, sta, o = _types(g, **kw)
    smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], o, np.float32(0))
    out["qsim"], out["cost"] = o.qsim.copy(), o.cost
    out.update({"fstates." + k: getattr(o.fstates, k).copy() for k in ss})
    setup, mesh, inp, par, sta, o = _types(g, **kw)
    par_b, sta_b = par.copy(), sta.copy()
    smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), o, o.copy(),
                        np.float32(0), np.float32(1))
    out["adj.cost"] = o.cost
    out.update({k + "_b": getattr(par_b, k).copy() for k in ps})
    out.update({k + "_b": getattr(sta_b, k).copy() for k in ss})
    plan = dict(inp._smashx_solver.timing(), **inp._smashx_solver.forcing_info())
    if tangent and g.direction is not None:
        setup, mesh, inp, par, sta, o = _types(g, **kw)
        par_d = smash_amd.ParametersDT.from_dict(mesh, g.direction)
        sta_d = smash_amd.StatesDT.from_dict(mesh, {k: np.zeros_like(v) for k, v in g.states.items()})
        o_d = smash_amd.OutputDT(setup, mesh)
        _, cost_d = smash_amd.forward_d(setup, mesh, inp, par, par_d, inp._bgd[0], par.copy(), sta, sta_d, inp._bgd[1], sta.copy(), o, o_d)
        out["qsim_d"], out["cost_d"] = o_d.qsim.copy(), cost_d
    print(f"plan: rounds {plan['n_rounds']} groups {plan['n_groups']} chained groups {plan['n_chained_groups']} max_stage "
          f"{plan['max_stage']} chain_staged {plan['chain_staged']} route_fwd_launches {plan['route_fwd_launches']} chunks "
          f"{plan['n_chunks']} x {plan['chunk_steps']} pipe {plan['pipe_steps']} layout {plan['layout'][:7]}")
    return out, plan


def _outputs(h):
    """Flat (name, array) pairs: discharge per gauge, the rest whole."""
    for k, v in h.items():
        if k in ("qsim", "qsim_d"):
            for i in range(np.asarray(v).shape[0]):
                yield f"{k}[{i}]", k, i
        else:
            yield k, k, None


def _check(cid, hip, ref):
    """Every output of hip against the oracle by the rules of the module docstring; returns the names that fail."""
    o32, o64 = ref[False], ref[True]
    exact = _exact()
    bad = []
    for name, k, i in _outputs(hip):
        h = np.asarray(hip[k], np.float64)
        r = o32[k]
        if i is not None:
            h, r = h[i], r[i]
        e_or = gu.rel_l2(h, r) if k not in SCALAR else abs(float(h) - float(r))
        if exact and k not in TANGENT:
            ok = np.array_equal(np.asarray(h, np.float32), np.asarray(r, np.float32))
            print(f"{cid} {name:14s} exact: {'bit-identical' if ok else 'DIFFERS'}  vs oracle32 {e_or:.2e}")
        else:
            t = o64[k] if i is None else o64[k][i]
            if k in SCALAR:
                e_hip, e_ref = abs(float(h) - float(t)), abs(float(r) - float(t))
                ok = e_hip <= 2.0 * e_ref + 3e-7
            else:
                e_hip, e_ref = gu.rel_l2(h, t), gu.rel_l2(r, t)
                ok = e_hip <= 2.0 * e_ref + 1e-6
            same = " (bit-identical)" if np.array_equal(np.asarray(h, np.float32), np.asarray(r, np.float32)) else ""
            print(f"{cid} {name:14s} e_hip {e_hip:.2e}  e_ref {e_ref:.2e}  ratio {e_hip / e_ref if e_ref else float('nan'):6.2f}  "
                  f"vs oracle32 {e_or:.2e}{same}")
            ok = ok or f"{cid}:{name}" in EXEMPT
        if not ok:
            bad.append(name)
    return bad


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("cid", ["W1", "W3", "W4", "W5", "L2", "L3", "L4"])
def test_sweep_at_size_vs_oracle(cid):
    """W1 gr-b 512^2 x 160 (+ tangent along cp, cft, lr): plan defaults, the chained launch over ~80 groups, plain rows.
    W3 gr-a on the 957 k cells of France x 48, nse + kge, the median over 12 of 16 gauges.  W4 vic-a 384^2 (D8) x 96, kge.
    W5 gr-c 384^2 x 96, nse + kge + logarithmic, prior + smoothing + hard_smoothing over normalised fields, denormalize_forward,
    optimize_start_step 13.  L2 gr-a 64^2 x 8760 from empty stores, kge.  L3 vic-a 48^2 x 8760 with 2 % data gaps.  L4 gr-d 48^2
    (D8) x 8760, rmse + kge2 from step 721 (a month of warm-up) (+ tangent)."""
    g, ref = _case(cid)
    t = time.time()
    hip, plan = _sweeps(g)
    print(f"{cid}: GPU sweeps {time.time() - t:.1f} s")
    if cid == "W1":
        _gpu_w1.update(hip)
        assert plan["n_chained_groups"] > 0 and plan["route_fwd_launches"] == 2, plan
        assert plan["chain_staged"] == 0 and plan["n_chunks"] == 1, plan
    if cid == "W3":
        assert plan["n_chained_groups"] > 0, plan
    bad = _check(cid, hip, ref)
    assert not bad, (cid, bad)


def test_staging_rows_by_the_plans_own_rule_at_size():
    """W2: W1's inputs with groups of 64 cells -- ~1350 chained groups, more than twice the compute units, so the plan puts the
    chained launches on staging rows BY ITS OWN RULE (SMASHX_CHAIN_STAGE unset) -- cut into 4 storage chunks of 48 steps (the last
    one ragged: 16) with pipeline sub-chunks of 16.  Every forward and adjoint output bit-identical to W1 (plan defaults) and, by
    W1's rules, to the oracle."""
    import os
    assert "SMASHX_CHAIN_STAGE" not in os.environ
    g, ref = _case("W1")
    if not _gpu_w1:
        _gpu_w1.update(_sweeps(g, tangent=False)[0])
    hip, plan = _sweeps(g, tangent=False, group_size=64, chunk_steps=48, pipe_steps=16)
    assert plan["n_chained_groups"] >= 2 * _cus(), (plan, _cus())
    assert plan["chain_staged"] == 1 and plan["n_chunks"] >= 3, plan
    for k, v in hip.items():
        assert np.array_equal(np.asarray(v), np.asarray(_gpu_w1[k])), k
    bad = _check("W2", hip, ref)
    assert not bad, bad


def test_full_year_store_all_and_compact_chunked():
    """L1: gr-b 64^2 x 8760, warm, nse.  Store-all with plan defaults (one storage chunk), and the compact forcing layout (uint16
    rain counts + daily PET) cut into at least 5 storage chunks (chunk_steps=1744: the plan makes 6 x 1472 steps, the last one
    ragged at 1400) with pipeline sub-chunks of 48: bit-identical to each other, both checked against the oracle."""
    g, ref = _case("L1")
    a, pa = _sweeps(g)
    assert pa["n_chunks"] == 1 and pa["layout"] == "fp32 rows", pa
    b, pb = _sweeps(g, layout=dict(SYNTH_LAYOUT), chunk_steps=1744, pipe_steps=48)
    assert pb["layout"].startswith("compact") and pb["n_chunks"] >= 5, pb
    assert 0 < pb["pipe_steps"] < pb["chunk_steps"], pb
    for k, v in a.items():
        assert np.array_equal(np.asarray(v), np.asarray(b[k])), k
    bad = _check("L1", a, ref)
    assert not bad, bad
