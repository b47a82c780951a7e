"""CPU: the cases of tests/bounds_cases.py (one field at a bound of the calibration box, states outside it) on the plain-C oracle,
before tests/test_gpu_bounds.py holds the HIP kernels to it there.

  * every output of the fp32 and of the fp64 oracle is finite on every case -- discharge, cost, final states, every gradient field,
    qsim_d, cost_d -- the four overflow corners included, at their moved-in values (bounds_cases.MOVED_IN);
  * the branch census (orc_census, oracle/smash_oracle.h): every counter is reached by at least one case, and every case named for a
    regime reaches it (bounds_cases.EXPECTED / EXPECTED_OUTSIDE);
  * where oracle/_ref/ has been built: the oracle is BIT-IDENTICAL to the compiled reference on the gr-c, gr-a and vic-a cases,
    forward and adjoint (the comparison of tests/test_oracle_at_size_cpu.py), so that bit-identity to the oracle means bit-identity to
    the reference out here too."""
import numpy as np
import pytest

import bounds_cases as bc
import golden_util as gu
from oracle import pyoracle, refbind

_runs = {}


def _run(cid):
    """(case, fp32 outputs, fp64 outputs, fp32 census) of case cid, computed once."""
    if cid not in _runs:
        g = bc.build(cid)
        with np.errstate(all="ignore"):
            o32, census = bc.oracle_outputs(g, fp64=False)
            o64, _ = bc.oracle_outputs(g, fp64=True)
        _runs[cid] = (g, o32, o64, census)
    return _runs[cid]


@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_every_output_is_finite_in_both_precisions(structure):
    bad = []
    for cid in bc.ids(structure):
        g, o32, o64, _ = _run(cid)
        want = {"qsim", "cost", "adj.cost", "qsim_d", "cost_d"} | {"fstates." + k for k in gu.STRUCT_STATES[structure]} \
            | {k + "_b" for k in bc.fields(structure)}
        assert want <= set(o32) and want <= set(o64), cid
        bad += [(cid, p, k) for p, o in (("fp32", o32), ("fp64", o64)) for k, v in o.items() if not np.all(np.isfinite(v))]
        assert np.any(o32["qsim"] != 0), cid
    assert not bad, bad


def test_every_census_counter_is_reached_by_some_case():
    reached = {k: [] for k in pyoracle.CENSUS}
    for cid in bc.ids():
        census = _run(cid)[3]
        assert set(census) == set(pyoracle.CENSUS) and census["cell_steps"] > 0, cid
        for k, v in census.items():
            if v:
                reached[k].append(cid)
        own = pyoracle.VIC_CENSUS if cid.split(":")[1] == "vic-a" else pyoracle.GR_CENSUS
        assert not [k for k in pyoracle.GR_CENSUS + pyoracle.VIC_CENSUS if k not in own and census[k]], cid
    for k, v in reached.items():
        print(f"{k:18s} {len(v):3d} cases, e.g. {v[0] if v else '-'}")
    assert not [k for k, v in reached.items() if not v], reached


def test_cases_reach_the_regime_they_are_named_for():
    missed = []
    for (field, end), (counters, structures) in bc.EXPECTED.items():
        for s in structures:
            census = _run(f"B:{s}:{field}:{end}")[3]
            missed += [(s, field, end, k) for k in counters if not census[k]]
    for s, counters in bc.EXPECTED_OUTSIDE.items():
        census = _run(f"O:{s}")[3]
        missed += [(s, "outside", k) for k in counters if not census[k]]
    assert not missed, missed
    for s in ("gr-a", "gr-b", "gr-c"):          # exc = -50 closes the direct branch on cell-steps where exc = +50 leaves it open
        assert _run(f"B:{s}:exc:lb")[3]["qd_zero"] > _run(f"B:{s}:exc:ub")[3]["qd_zero"], s


def test_moved_in_values_are_inside_the_box():
    for (field, end) in bc.MOVED_IN:
        lo, hi = (refbind.GLB_P, refbind.GUB_P) if field in bc.synth.PARAM_NAMES else (refbind.GLB_S, refbind.GUB_S)
        i = (bc.synth.PARAM_NAMES if field in bc.synth.PARAM_NAMES else bc.synth.STATE_NAMES).index(field)
        assert lo[i] < bc.bound_value(field, end) < hi[i], (field, end)


def _same(a, b):
    """Bit for bit as fp32 values; a NaN equals a NaN in the same place."""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def _against_the_reference(cid):
    """Names of the outputs of case cid on which the oracle is not bit-identical to the compiled reference, forward and adjoint.

    base_forward_b: the oracle as it stands.  base_forward: the oracle with MAX / MIN evaluated as the reference's build evaluates
    the intrinsics of the original operators (pyoracle.run(reference_max=True), oracle/smash_oracle.c) -- and, wherever the
    reference's forward outputs are finite, also the oracle as it stands: the two evaluations agree on ordered operands.  Where they
    are not finite (see test_oracle_is_the_reference_outside_the_box) the oracle as it stands must instead return, from its forward
    run, the discharge and cost of its adjoint run, which ARE the reference's base_forward_b bit for bit."""
    g = bc.build(cid)
    ps, ss = gu.STRUCT_PARAMS[g.structure], gu.STRUCT_STATES[g.structure]
    a = (g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
    bad = []
    with np.errstate(all="ignore"):
        o = pyoracle.run(*a, **g.opts)
        om = pyoracle.run(*a, reference_max=True, **g.opts)
        ob = pyoracle.run(*a, adjoint=True, **g.opts)
    r = refbind.run(*a, fast=False, **g.opts)
    rb = refbind.run(*a, adjoint=True, fast=False, **g.opts)
    fwd = lambda x: [("qsim", x["qsim"]), ("cost", x["cost"]), ("cost_jobs", x["cost_jobs"])] + [("fstates." + k, x["fstates"][k]) for k in ss]
    bad += [(cid, "ref-max " + k) for (k, u), (_, v) in zip(fwd(om), fwd(r)) if not _same(u, v)]
    if all(np.all(np.isfinite(v)) for _, v in fwd(r)):
        bad += [(cid, k) for (k, u), (_, v) in zip(fwd(o), fwd(r)) if not _same(u, v)]
    else:
        bad += [(cid, "fwd-vs-adj " + k) for k in ("qsim", "cost", "cost_jobs") if not _same(o[k], ob[k])]
    bad += [(cid, "adj." + k) for k in ("qsim", "cost", "cost_jobs") if not np.array_equal(np.float32(ob[k]), np.float32(rb[k]))]
    bad += [(cid, k + "_b") for k in ps if not np.array_equal(ob["parameters_b"][k], rb["parameters_b"][k])]
    bad += [(cid, k + "_b") for k in ss if not np.array_equal(ob["states_b"][k], rb["states_b"][k])]
    assert np.any(o["qsim"] != 0) and np.isfinite(o["cost"]) and np.isfinite(ob["cost"]), cid
    return bad


needs_ref = pytest.mark.skipif(not refbind.available(False), reason="oracle/_ref/libsmash_ref.so not built")


@needs_ref
@pytest.mark.parametrize("structure", ["gr-c", "gr-a", "vic-a"])
def test_oracle_is_the_reference_at_the_bounds(structure):
    """Every B: case of the structure, forward and adjoint, every output bit-identical (and finite in the reference: the oracle as it
    stands is compared on all of them)."""
    bad = []
    for cid in bc.ids(structure):
        if cid.startswith("B:"):
            bad += _against_the_reference(cid)
            g = bc.build(cid)
            r = refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, fast=False)
            assert np.all(np.isfinite(r["qsim"])) and np.isfinite(r["cost"]), cid
    assert not bad, bad


@needs_ref
@pytest.mark.parametrize("structure", ["gr-c", "vic-a"])
def test_oracle_is_the_reference_outside_the_box(structure):
    """The O: case of the structure, forward and adjoint, every output bit-identical.

    On O:gr-c the reference disagrees with ITSELF.  On the 3 cells that are in a data gap at the first step with hft = 1.2,
    (ht ct)^-4 - ct^-4 < 0 and its power -1/4 is NaN.  md_gr_operator.f90:104 floors it with the MAX intrinsic, max(1.e-6, NaN), which
    the flang build evaluates to NaN (the standard leaves it to the processor): base_forward returns hft = NaN on those cells and NaN
    discharge and cost.  forward_db.f90:6444-6448, the copy of gr_transfer that base_forward_b runs, states the same floor as
    IF (1.e-6 < x) ... ELSE ht_imd = 1.e-6, which takes the floor: base_forward_b returns finite discharge, cost and gradients.  The
    oracle restates both: as it stands it takes the floor (C's fmaxf; so do the HIP kernels) and is base_forward_b bit for bit,
    discharge and cost included, in its forward run too; with orc_set_reference_max(1) it evaluates MAX as the build does and is
    base_forward bit for bit, the NaN in the same places (_against_the_reference)."""
    bad = _against_the_reference(f"O:{structure}")
    assert not bad, bad
