"""Records tests/golden/jreg_edges/jreg_edges.npz: what the compiled reference (oracle/refbind.run -> oracle/_ref/libsmash_ref.so, the parity
build) computes on the cases of tests/jreg_cases.py -- the regularisers at the edges of grid shape, mask and sum length -- in both
weightings: cost, cost_jobs, cost_jreg of the forward run, cost_d of the tangent run along the case's direction, and every gradient
plane of the adjoint run that is not identically zero (a plane that is absent is zero in the reference).  All float32, keys
<id>.<weighting>.<name> (jreg_cases.recorded).  The file holds numbers only.

    python tests/golden/make_jreg_edges.py        # needs oracle/_ref (built from the reference by __graft_entry__.build())
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "jreg_edges", "jreg_edges.npz")


def record():
    import jreg_cases as jc
    from oracle import refbind
    d = {}
    for cid in jc.IDS:
        for w in jc.WEIGHTINGS:
            r = jc.recorded(jc.build(cid, w), refbind.run)
            d.update(r)
            pre = f"{cid}.{w}."
            print(f"{pre[:-1]:22s} cost {r[pre + 'cost']:.9g} jobs {r[pre + 'cost_jobs']:.9g} jreg {r[pre + 'cost_jreg']:.9g} cost_d "
                  f"{r[pre + 'cost_d']:.9g} planes {sorted(k[len(pre):] for k in r if k.endswith('_b'))}")
    return d


if __name__ == "__main__":
    d = record()
    np.savez_compressed(OUT, **d)
    print(f"{OUT}: {len(d)} entries, {os.path.getsize(OUT)} bytes")
