"""CPU: the plain-C oracle (oracle/liboracle.so, the reference of every GPU parity test) is pinned to the compiled reference
(oracle/_ref/libsmash_ref.so, the parity build) bit for bit at the golden-fixture sizes (tests/test_oracle_golden.py); here also at
size -- a reduced W1 of tests/test_gpu_parity_at_size.py (gr-b, 256^2 cells x 160 steps: deep routing trees, whole-grid sums) and a
reduced L2 (gr-a, 48^2 cells x 8760 steps from empty stores: a year of summation).  Forward and adjoint, every output BIT-IDENTICAL."""
import numpy as np
import pytest

import golden_util as gu
import size_cases as sc
from oracle import pyoracle, refbind

pytestmark = pytest.mark.skipif(not refbind.available(False), reason="oracle/_ref/libsmash_ref.so not built")


@pytest.mark.parametrize("cid", ["W1s", "L2s"])
def test_oracle_is_the_reference_at_size(cid):
    g = sc.build(cid)
    a = (g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
    for adjoint in (False, True):
        o = pyoracle.run(*a, adjoint=adjoint, **g.opts)
        r = refbind.run(*a, adjoint=adjoint, fast=False, **g.opts)
        bad = [k for k in ("qsim", "cost", "cost_jobs") if not np.array_equal(np.float32(o[k]), np.float32(r[k]))]
        if adjoint:
            bad += [k + "_b" for k in gu.STRUCT_PARAMS[g.structure] if not np.array_equal(o["parameters_b"][k], r["parameters_b"][k])]
            bad += [k + "_b" for k in gu.STRUCT_STATES[g.structure] if not np.array_equal(o["states_b"][k], r["states_b"][k])]
        else:
            bad += ["fstates." + k for k in gu.STRUCT_STATES[g.structure] if not np.array_equal(o["fstates"][k], r["fstates"][k])]
        assert not bad, (cid, adjoint, bad)
        assert np.any(o["qsim"] != 0) and np.isfinite(o["cost"])
