"""Records tests/golden/multiple_run/gr_a_cance_s16.npz: 16 samples of the Cance case (gr-a, 383 cells x 1440 steps) through the
compiled reference (oracle/refbind.run, one forward per sample as mw_multiple_run.f90:96-117 does), so that
tests/test_gpu_ensemble.py can check smashx_multiple_run against the reference where oracle/_ref is absent.

Stored: sample (nf, 16), ind (nf, 1-based stacked md_constant order), names, res_cost (16), res_qsim (ng, nt, 16) and the
reference's own flag-to-flag noise on them (its -O3 + FMA build against the parity build).  The script refuses a seed for which
a cost is not finite or the noise on the costs exceeds the cost noise recorded in the Cance fixture; it also prints the noise on
the discharge series (samples drawn over the whole default bounds are touchier than the calibrated fields of the fixture).

    python tests/golden/make_multiple_run.py [seed]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import golden_util as gu            # noqa: E402
import multiple_run_util as mu      # noqa: E402
from oracle import refbind          # noqa: E402

CASE, S = "gr_a_cance_28x28x1440", 16


def main(seed):
    g = gu.load(CASE)
    names = mu.fields_of(g.structure)
    sample = mu.draw(names, S, seed)
    cost = np.zeros(S, np.float32)
    qsim = np.zeros((g.mesh.ng, g.nt, S), np.float32, order="F")
    ncost, nq = np.zeros(S), np.zeros((g.mesh.ng, S))
    for i in range(S):
        p, s = mu.filled(g.params, names, sample[:, i]), mu.filled(g.states, names, sample[:, i])
        r = refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, p, s, **g.opts)
        f = refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, p, s, fast=True, **g.opts)
        cost[i], qsim[:, :, i] = r["cost"], r["qsim"]
        ncost[i] = abs(f["cost"] - r["cost"]) / abs(r["cost"])
        nq[:, i] = [gu.rel_l2(f["qsim"][k], r["qsim"][k]) for k in range(g.mesh.ng)]
    print("seed", seed, "costs", cost)
    print("noise: cost max %.3e (fixture %.3e), qsim max per gauge %s (fixture %s)" % (ncost.max(), g.noise["cost"], nq.max(axis=1), g.noise["qsim"]))
    ok = bool(np.all(np.isfinite(cost)) and np.all(np.isfinite(qsim)) and ncost.max() <= g.noise["cost"])
    if not ok:
        print("REFUSED: a cost is not finite or the reference's own noise on the costs exceeds the fixture's; try another seed")
        return 1
    out = os.path.join(HERE, "multiple_run", "gr_a_cance_s16.npz")
    np.savez_compressed(out, case=CASE, seed=seed, names=np.array(names), ind=mu.index_of(names), sample=sample, res_cost=cost,
                        res_qsim=qsim, noise_cost=ncost, noise_qsim=nq)
    print("wrote", out, os.path.getsize(out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else mu.SEED))
