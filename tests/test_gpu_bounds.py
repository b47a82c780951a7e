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
structure are in one test: 12 x 12 x 72 sweeps are milliseconds, the time is plan creation."""
import time

import numpy as np
import pytest

import bounds_cases as bc
from test_gpu_parity_at_size import _check, _sweeps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_sweeps_at_the_bounds_vs_oracle(structure):
    t = time.time()
    cases = []
    for cid in bc.ids(structure):
        g = bc.build(cid)
        with np.errstate(all="ignore"):
            ref = {f64: bc.oracle_outputs(g, fp64=f64)[0] for f64 in (False, True)}
        cases.append((g, ref))
    print(f"{structure}: {len(cases)} cases, oracle {time.time() - t:.1f} s")
    t = time.time()
    bad = []
    for g, ref in cases:
        hip, plan = _sweeps(g)
        assert plan["n_chunks"] == 1, (g.id, plan)
        bad += [(g.id, b) for b in _check(g.id, hip, ref)]
        chunked, plan = _sweeps(g, tangent=False, chunk_steps=32, pipe_steps=16)
        assert plan["n_chunks"] >= 2 and 0 < plan["pipe_steps"] < plan["chunk_steps"], (g.id, plan)
        bad += [(g.id, "chunked " + k) for k, v in chunked.items() if not np.array_equal(np.asarray(v), np.asarray(hip[k]), equal_nan=True)]
    print(f"{structure}: GPU sweeps {time.time() - t:.1f} s")
    assert not bad, bad
