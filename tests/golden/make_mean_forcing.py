"""Records tests/golden/mean_forcing/<case>.npz: the catchment-mean forcing the compiled reference forms
(mw_forcing_statistic::compute_mean_forcing, smash/solver/routine/mw_forcing_statistic.f90:18-75) on the forcing of existing fixtures,
so that tests/test_mean_forcing_cpu.py can pin the numpy restatement (tests/mean_forcing_util.py) and tests/test_gpu_mean_forcing.py
the library against the reference where oracle/_ref is absent.

oracle/ref/ref_capi.f90 has no entry for this routine; tests/golden/mean_forcing_driver.f90 is a bind(C) driver of our own.  It is
compiled here against the module files and objects oracle/ref/build_ref.sh leaves in oracle/_ref/obj_parity, with the same flags
(-O2 -ffp-contract=off), into a temporary directory: nothing compiled is kept.

Stored per case: mean_prcp, mean_pet (ng, nt) and the description of the variant (the golden case, the blanked steps).  The forcing is
the golden case's and is not stored again.  Every case is also run with sparse storage (the reference's other branch must agree bit for
bit, NaN = NaN) and must show at least MIN_SEQUENTIAL (gauge, step) pairs on which the sequential fp32 sum differs from the fp64 sum
rounded once, or the script refuses it.

    python tests/golden/make_mean_forcing.py [--time]      (--time: also print the routine's time on the Cance case, best of 5)
"""
import ctypes as C
import glob
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)

import golden_util as gu             # noqa: E402
import mean_forcing_util as mu       # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj_parity")
MIN_SEQUENTIAL = 8


def build(tmp):
    """the driver + the reference's objects -> tmp/libmf.so"""
    if not os.path.exists(os.path.join(OBJ, "mw_forcing_statistic.mod")):
        raise SystemExit(f"{OBJ} lacks mw_forcing_statistic.mod: run __graft_entry__.build() where the reference is present")
    flags = ["-cpp", "-O2", "-ffp-contract=off", "-fPIC"]
    obj = os.path.join(tmp, "mean_forcing_driver.o")
    subprocess.check_call([FC] + flags + ["-module-dir", tmp, "-I" + OBJ, "-c", os.path.join(HERE, "mean_forcing_driver.f90"), "-o", obj])
    lib = os.path.join(tmp, "libmf.so")
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "ref_capi.o"]
    subprocess.check_call([FC, "-shared", "-o", lib, obj] + others)
    return C.CDLL(lib)


def run(lib, g, prcp, pet, sparse, nrep=1):
    m = g.mesh
    gp = np.asarray(m.gauge_pos).reshape(-1, 2)
    ng = gp.shape[0]
    icfg = np.array([m.nrow, m.ncol, g.nt, ng, int(sparse), nrep], np.int32)
    flw = np.asfortranarray(m.flwdir, dtype=np.int32)
    path = np.asfortranarray(np.asarray(m.path) + 1, dtype=np.int32)
    act = np.asfortranarray(m.active_cell, dtype=np.int32)
    gpos = np.asfortranarray(gp + 1, dtype=np.int32)
    prcp, pet = np.asfortranarray(prcp, dtype=np.float32), np.asfortranarray(pet, dtype=np.float32)
    mp = np.full((ng, g.nt), -7.0, np.float32, order="F")
    me = np.full((ng, g.nt), -7.0, np.float32, order="F")
    elapsed = C.c_double(0.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    lib.mf_run.restype = None
    lib.mf_run(p(icfg), p(flw), p(path), p(act), p(gpos), p(prcp), p(pet), p(mp), p(me), C.byref(elapsed))
    return mp, me, elapsed.value


def main(timed):
    os.makedirs(mu.DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for name, case in mu.CASES.items():
            g = gu.load(case)
            m = g.mesh
            prcp, pet = mu.blanked(name, g.prcp, g.pet)
            act = np.asarray(m.active_cell) == 1
            masks = mu.gauge_masks(m)
            assert all(np.all(act[k]) for k in masks), f"{name}: an upstream mask leaves the active cells (the sparse branch is undefined there)"
            mp, me, _ = run(lib, g, prcp, pet, sparse=False)
            sp, se, _ = run(lib, g, prcp, pet, sparse=True)
            assert mu.same_bits(mp, sp) and mu.same_bits(me, se), f"{name}: the reference's dense and sparse branches disagree"
            mine = mu.mean_forcing(m.flwdir, m.gauge_pos, prcp, pet)
            wide = mu.fp64_means(m.flwdir, m.gauge_pos, prcp, pet)
            nseq = mu.count_differing(mp, wide[0]) + mu.count_differing(me, wide[1])
            print(f"{name}: catchments of {[int(k.sum()) for k in masks]} cells, {g.nt} steps, NaN steps prcp {int(np.isnan(mp).sum())} pet {int(np.isnan(me).sum())}, "
                  f"numpy restatement differs on {mu.count_differing(mp, mine[0])} + {mu.count_differing(me, mine[1])} of {mp.size} + {me.size}, "
                  f"the fp64 sum rounded once differs on {nseq}")
            if nseq < MIN_SEQUENTIAL:
                print(f"REFUSED: {name} tells a sequential sum from a reassociated one on {nseq} < {MIN_SEQUENTIAL} values: pick another case")
                return 1
            b = mu.BLANK.get(name, dict(prcp=(), pet=()))
            out = os.path.join(mu.DIR, name + ".npz")
            np.savez_compressed(out, case=case, blank_prcp=np.array(b["prcp"], np.int32), blank_pet=np.array(b["pet"], np.int32),
                                mean_prcp=mp, mean_pet=me)
            print("wrote", out, os.path.getsize(out), "bytes")
        if timed:
            g = gu.load("gr_a_cance_28x28x1440")
            _, _, sec = run(lib, g, g.prcp, g.pet, sparse=False, nrep=5)
            cells = sum(int(k.sum()) for k in mu.gauge_masks(g.mesh))
            cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), platform.processor())
            print(f"reference routine on gr_a_cance_28x28x1440 (one core of {cpu}, -O2 -ffp-contract=off, best of 5): {sec:.5f} s for "
                  f"{g.mesh.nrow * g.mesh.ncol} grid cells x {g.nt} steps x {np.asarray(g.mesh.gauge_pos).reshape(-1, 2).shape[0]} gauges x 2 fields "
                  f"({cells} masked cells per step and field)")
    return 0


if __name__ == "__main__":
    sys.exit(main("--time" in sys.argv[1:]))
