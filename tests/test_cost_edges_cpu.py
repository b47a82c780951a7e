"""CPU: the gauge cost stage at its edges (tests/cost_edge_cases.py).

  * the numpy restatement of compute_jobs / COMPUTE_JOBS_B / COMPUTE_JOBS_D in sequential fp32 equals what the compiled reference
    recorded in tests/golden/cost_edges/cost_edges.npz bit for bit (in NaN-ness where not finite), on every recorded case and for both
    seeds; the module rebuilds the recorded inputs bit for bit;
  * where oracle/_ref is present, a fresh run of tests/golden/cost_edges_driver.f90 over the reference equals the fixture bit for bit;
  * a gauge with a non-zero weight and no observation from the start step on counts as weight 0: on the oracle, every output of the
    forward, adjoint and tangent runs equals the run with that weight set to 0 bit for bit, and cost_d agrees with <gradient,
    direction> as closely as it does then (before the rule: 1.01554 against 2.03109 on "second")."""
import os
import sys
import tempfile

import numpy as np
import pytest

import cost_edge_cases as ce
import jreg_cases as jc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIX = ce.load_fixture()
CASES = ce.cases()


def test_the_fixture_holds_exactly_the_cases_of_the_module():
    assert list(FIX) == list(CASES)
    assert os.path.getsize(ce.FIXTURE) < 512 * 1024


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_in_fp32_equals_the_reference(name):
    c, r = CASES[name], FIX[name]
    for k in ce.INPUTS:
        assert np.array_equal(np.asarray(c[k]).view(np.uint32) if c[k].dtype == np.float32 else c[k],
                              np.asarray(r[k]).view(np.uint32) if r[k].dtype == np.float32 else r[k]), k
    assert c["jobs"] == r["jobs_fun"] and c["start"] == r["start"]
    m1, m2 = ce.restate(c, jobs_b=ce.JOBS_B[0]), ce.restate(c, jobs_b=ce.JOBS_B[1])
    print(name, "jobs", m1["jobs"], r["jobs"], "jobs_d", m1["jobs_d"], r["jobs_d"], "n", sorted(set(int(v) for v in m1["n"])))
    assert ce.same_bits(m1["jobs"], r["jobs"]) and ce.same_bits(m1["jobs_d"], r["jobs_d"])
    assert ce.same_bits(m1["qsim_b"], r["qsim_b1"]) and ce.same_bits(m2["qsim_b"], r["qsim_b2"])
    assert list(m1["n"]) == list(c["claims"]["n"])
    # the seeds are exactly 0 before the start step, on missing steps and on the gauges that get none
    s0 = c["start"] - 1
    qo = ce.normalised(c)[0]
    for b in (r["qsim_b1"], r["qsim_b2"]):
        assert not b[:, :s0].any() and not b[:, s0:][qo[:, s0:] < 0].any() and not b[c["wgauge"] == 0].any()
        if np.any(c["wgauge"] < 0):
            assert not b[c["wgauge"] > 0].any()


def test_three_quarters_of_the_criteria_are_finite_in_the_reference():
    flags = [f for r in FIX.values() for f in r["finite"].values()]
    assert 4 * sum(flags) >= 3 * len(flags) and not all(flags), (sum(flags), len(flags))
    # and the fp64 restatement agrees with the reference where it is finite (a loose bar: it only shows that both state one formula)
    for name in ("len129", "gaps_alternating", "njf8", "median5", "g70"):
        t = ce.restate(CASES[name], np.float64)
        assert abs(float(t["jobs"]) - float(FIX[name]["jobs"])) <= 1e-4 * abs(float(t["jobs"])), name
        assert abs(float(t["jobs_d"]) - float(FIX[name]["jobs_d"])) <= 1e-3 * abs(float(t["jobs_d"])), name


def test_tie_cases_hand_the_seed_to_another_gauge_than_a_stable_sort():
    for name, c in CASES.items():
        if c["claims"].get("tie") == "at":
            tied, pts, seeded, stable = ce.tie_report(c, ce.restate(c))
            got = tuple(int(g) for g in np.flatnonzero(np.any(FIX[name]["qsim_b1"] != 0, axis=1)))
            assert got == seeded and seeded != stable and set(pts) & set(tied), (name, got, seeded, stable)


def test_fresh_run_of_the_driver_equals_the_fixture():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "obj_parity", "mwd_cost_diff.mod")):
        pytest.skip("oracle/_ref is not built here (the reference is absent)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_cost_edges as mk
    with tempfile.TemporaryDirectory() as tmp:
        lib = mk.build(tmp)
        for name, c in CASES.items():
            ref = mk.run(lib, c)
            for k, v in ref.items():
                assert ce.same_bits(v, FIX[name][k]), (name, k)


# ---- gauges without data: the oracle --------------------------------------------------------------------------------------------------------
def _flat(g):
    from oracle import pyoracle
    fwd, adj, tan = jc.run_all(g, pyoracle.run)
    out = dict(qsim=fwd["qsim"], cost=fwd["cost"], cost_jobs=fwd["cost_jobs"], cost_jreg=fwd["cost_jreg"])
    out.update({"fstates." + k: v for k, v in fwd["fstates"].items()})
    out["adj.cost"], out["adj.cost_jobs"] = adj["cost"], adj["cost_jobs"]
    out.update(jc.planes(adj))
    out["qsim_d"], out["cost_d"], out["tan.cost_jobs"] = tan["qsim_d"], tan["cost_d"], tan["cost_jobs"]
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def _along(g, flat):
    """<gradient, direction> in double"""
    d = dict(g.direction[0], **g.direction[1])
    return float(sum(np.sum(flat[k + "_b"] * np.asarray(v, np.float64)) for k, v in d.items()))


@pytest.mark.parametrize("name", list(ce.SWEEP_EMPTY))
def test_oracle_counts_a_gauge_without_data_as_weight_zero(name):
    gw, gz = ce.sweep_case(name), ce.sweep_case(name, zero=True)
    w, z = _flat(gw), _flat(gz)
    bad = [k for k in w if not ce.same_bits(w[k], z[k])]
    gap_w, gap_z = abs(float(w["cost_d"]) - _along(gw, w)), abs(float(z["cost_d"]) - _along(gz, z))
    print(name, "cost", float(w["cost"]), "cost_jobs", float(w["cost_jobs"]), "cost_d", float(w["cost_d"]), "<gradient, direction>", _along(gw, w),
          "with the weight at 0:", float(z["cost_d"]), _along(gz, z))
    assert not bad, bad
    assert gap_w == gap_z            # (follows from the equality above; the bars are the next one and the regression test)
    if name != "both":          # ("both": the regulariser's fp32 sums alone are left, 1e-3 of a cost_d of 1e-5)
        assert gap_z <= 1e-4 * abs(float(z["cost_d"]))
        assert float(w["cost_jobs"]) != 0.0 and any(np.any(w[k + "_b"]) for k in ("cp", "hlr"))


def test_the_regression_the_rule_was_decided_on():
    """two gauges, the second without data, wgauge = (0.5, 0.5), nse alone: before the rule the adjoint carried the empty gauge's seed
    into gauge 1 and <gradient, direction> was twice cost_d"""
    g = ce.sweep_case("second", jobs=dict(jobs_fun=("nse",), wjobs_fun=(1.0,)))
    w = _flat(g)
    assert abs(_along(g, w) - float(w["cost_d"])) <= 1e-4 * abs(float(w["cost_d"])), (_along(g, w), float(w["cost_d"]))
