#!/usr/bin/env python3
"""tests/golden/vertical_forms/noise.npz: the reference's own flag-to-flag noise on every output of every case of
tests/test_gpu_vertical_forms.py (the golden fixtures with the forcing cut short, tests/vertical_forms_cases.py), measured the way
make_golden.py measures it for the fixtures themselves: the UNMODIFIED reference solver built as its makefile does (-O3 + FMA)
against its parity build (-O2 -ffp-contract=off), both from oracle/ref/build_ref.sh.  Data only: one float64 per (case, output).

Run in the build container (needs the reference binaries under oracle/_ref/):   python tests/golden/vertical_forms/make_noise.py
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as gu  # noqa: E402
import vertical_forms_cases as vc  # noqa: E402
from oracle import refbind  # noqa: E402


def noise(a, b):
    """rel-L2 distance of a from b over the values finite in both (a criterion over one or two steps can be 0 / 0)"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    fin = np.isfinite(a) & np.isfinite(b)
    return float(gu.rel_l2(a[fin], b[fin])) if fin.any() else 0.0


def main():
    d = {}
    for name, nt, pattern in vc.all_cases():
        g = vc.make(name, nt, pattern)
        run = lambda **kw: refbind.run(g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, **g.opts, **kw)
        par, fast = vc.outputs(g.structure, run(), run(adjoint=True)), vc.outputs(g.structure, run(fast=True), run(adjoint=True, fast=True))
        for k in par:
            d[vc.key(name, nt, pattern, k)] = np.float64(noise(fast[k], par[k]))
        print(name, nt, pattern, {k: f"{d[vc.key(name, nt, pattern, k)]:.1e}" for k in par})
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "noise.npz"), **d)


if __name__ == "__main__":
    main()
