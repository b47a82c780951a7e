"""GPU: the sweeps at the bounds of the calibration box against the CPU oracle.  Everything else in the suite runs the kernels in the
middle of the feasible box; the cases of tests/bounds_cases.py put one field of the structure on a bound (or states outside the box)
and so run the operators of sx_ops.h, sx_vic.h, sx_tangent.h and the routing kernels on the edges of their shortcuts: saturated tanh,
powers at the 1e-6 floor, the gap branch with a non-positive base, the percolation power above |hp| = 15 that the still-step test must
not skip, ci and lr at both ends, the clamps of the vic-a operators.  tests/test_bounds_cpu.py shows on the oracle's branch census that
the cases reach those branches.

Forward, adjoint and tangent of every case through smash_amd.forward / forward_b / forward_d, by the rules of
tests/test_gpu_parity_at_size.py, unchanged (its _sweeps and _check):
  * exact-libm build (SMASHX_EXACT_LIBM=1, run by tests/test_gpu_exact.py): every forward and adjoint output BIT-IDENTICAL to the fp32
    oracle -- discharge per gauge, cost, final states, every gradient field;
  * default build, and the tangent outputs in both builds: rel_l2(hip, truth64) <= 2 rel_l2(oracle32, truth64) + 1e-6 per output,
    costs |hip - truth| <= 2 |ref - truth| + 3e-7; truth64 = the same statements in double.
Every output prints one line.  Each case also runs forward and adjoint with a small storage chunk (chunk_steps=32, pipe_steps=16: the
adjoint rebuilds the states from checkpoints at the bounds), bit-identical to the store-all run of the same build.  All cases of a
structure are in one test: 12 x 12 x 72 sweeps are milliseconds, the time is plan creation.

The composite tangent direction of a case (1 % of every parameter) hides the weak fields behind the strong ones, and on gr-b and gr-c
its bar is loose: along ci the fp32 oracle sits on the interception kink at PET = 0, 5 .. 40 % away from the fp64 truth, which lifts
the composite e_ref to 1e-4 .. 1e-3 (tests/tangent_field_cases.py).  So every case runs further tangent sweeps on one more plan
(bounds_cases.tangent_extras), the composite check staying as it is:
  * gr-b, gr-c: the composite direction without ci, by the same _check rule (e_ref 3e-7 .. 5e-6);
  * every B: case: the direction of the field ON THE BOUND alone, parameter or state.  The adjoint-tangent identity against the
    gradient of the adjoint sweep that _sweeps ran, gap_hip <= 2 gap_ref32 + 2e-5 scale (tests/test_gpu_tangent_fields.py); the _check
    rule too where the fp32 oracle is within 1e-4 of the truth along that direction (all but 13 of the 92 cases:
    tests/test_tangent_fields_cpu.py);
  * the ci and hi cases of gr-b and gr-c: that direction once more on a copy of the case with the zeros of PET at 0.013, identity
    (against an adjoint sweep of the copy) and _check rule."""
import time

import numpy as np
import pytest

import bounds_cases as bc
import tangent_field_cases as tf
from test_gpu_parity_at_size import _check, _sweeps

pytestmark = pytest.mark.gpu


def _extra_tangents(extras, hip, o32):
    """The sweeps of bounds_cases.tangent_extras: one plan per case (g, its floor copy), every direction of the case on it.  hip, o32:
    the outputs of _sweeps and of the fp32 oracle on g, whose gradients serve the identity.  Returns the names that fail."""
    bad, sweeps = [], {}
    for label, case, direction, field, ref32, ref64, grad32, truth in extras:
        if case.id not in sweeps:
            sweeps[case.id] = tf.Sweeps(case)
        t = sweeps[case.id].tangent(direction)
        if field is not None:
            own = grad32 is None                        # (a floor copy has gradients of its own, on both sides)
            b, _ = tf.identity_failures(label, t["cost_d"], hip[field + "_b"] if own else sweeps[case.id].gradient()[field], ref32,
                                        o32[field + "_b"] if own else grad32, tf.plane(direction, field))
            bad += b
        if truth:
            bad += [f"{label} {b}" for b in _check(label, {k: t[k] for k in ("qsim_d", "cost_d")}, {False: ref32, True: ref64})]
        else:
            print(f"{label}: fp32 oracle {max(tf.e_ref(ref32, ref64)):.2e} from the truth, identity only")
    return bad


@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_sweeps_at_the_bounds_vs_oracle(structure):
    t = time.time()
    cases = []
    for cid in bc.ids(structure):
        g = bc.build(cid)
        with np.errstate(all="ignore"):
            ref = {f64: bc.oracle_outputs(g, fp64=f64)[0] for f64 in (False, True)}
            extras = bc.tangent_extras(g)
        cases.append((g, ref, extras))
    print(f"{structure}: {len(cases)} cases, oracle {time.time() - t:.1f} s")
    t = time.time()
    bad = []
    for g, ref, extras in cases:
        hip, plan = _sweeps(g)
        assert plan["n_chunks"] == 1, (g.id, plan)
        bad += [(g.id, b) for b in _check(g.id, hip, ref)]
        chunked, plan = _sweeps(g, tangent=False, chunk_steps=32, pipe_steps=16)
        assert plan["n_chunks"] >= 2 and 0 < plan["pipe_steps"] < plan["chunk_steps"], (g.id, plan)
        bad += [(g.id, "chunked " + k) for k, v in chunked.items() if not np.array_equal(np.asarray(v), np.asarray(hip[k]), equal_nan=True)]
        bad += [(g.id, b) for b in _extra_tangents(extras, hip, ref[False])]
    print(f"{structure}: GPU sweeps {time.time() - t:.1f} s")
    assert not bad, bad
