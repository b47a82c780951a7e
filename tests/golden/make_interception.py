"""Records tests/golden/interception/<case>.npz: the interception capacities the compiled reference chooses
(mw_interception_store::adjust_interception_store, smash/solver/routine/mw_interception_store.f90:19-160) on the forcing of existing
fixtures, so that tests/test_interception_cpu.py can pin the numpy restatement (tests/interception_util.py) and
tests/test_gpu_interception.py the library against the reference where oracle/_ref is absent.

oracle/ref/ref_capi.f90 has no entry for this routine; tests/golden/interception_driver.f90 is a bind(C) driver of our own.  It is
compiled here against the module files and objects oracle/ref/build_ref.sh leaves in oracle/_ref/obj_parity, with the same flags
(-O2 -ffp-contract=off), into a temporary directory: nothing compiled is kept.

Stored per case: day_index (nt), nday, start_time, structure (the one the case was recorded as) and the ci plane (nrow, ncol): the
routine's result on active cells, SENTINEL elsewhere.  The forcing is the golden case's and is not stored again.  day_index is built
with the reference's own statements (smash/core/_build_model.py:238-248, pandas) for a run of nt steps from start_time.  Every case is
also run with sparse storage (the reference's other branch must agree bit for bit) and must show at least MIN_DISTINCT distinct
capacities on active cells, or the script refuses it.

    python tests/golden/make_interception.py [--time]      (--time: also print the routine's time on the Cance case, best of 5)
"""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)

import golden_util as gu            # noqa: E402
import interception_util as iu      # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj_parity")
SENTINEL = np.float32(-7.0)
MIN_DISTINCT = 5
# fixture -> (structure id of the run, start_time)
RUNS = {
    "gr_b_16x16x96_nse_gaps": (2, "2014-09-15 00:00"),
    "gr_b_16x16x96_nse_gaps__start17": (2, "2014-09-15 17:00"),
    "gr_c_32x32x240_d8_ragged": (3, "2014-09-15 00:00"),
    "gr_a_cance_28x28x1440": (2, "2014-09-15 00:00"),
}


def build(tmp):
    """the driver + the reference's objects -> tmp/libici.so"""
    if not os.path.exists(os.path.join(OBJ, "mw_interception_store.mod")):
        raise SystemExit(f"{OBJ} lacks mw_interception_store.mod: run __graft_entry__.build() where the reference is present")
    flags = ["-cpp", "-O2", "-ffp-contract=off", "-fPIC"]
    obj = os.path.join(tmp, "interception_driver.o")
    subprocess.check_call([FC] + flags + ["-module-dir", tmp, "-I" + OBJ, "-c", os.path.join(HERE, "interception_driver.f90"), "-o", obj])
    lib = os.path.join(tmp, "libici.so")
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "ref_capi.o"]
    subprocess.check_call([FC, "-shared", "-o", lib, obj] + others)
    return C.CDLL(lib)


def reference_day_index(start_time, nt, dt):
    """smash/core/_build_model.py:238-248, for a run of nt steps"""
    start = pd.Timestamp(start_time)
    end = start + pd.Timedelta(seconds=int(dt) * nt)
    date_range = pd.date_range(start=start, end=end, freq=f"{int(dt)}s")[1:].strftime("%Y%m%d")
    n = 1
    day_index = np.ones(shape=len(date_range), dtype=np.int64)
    for i in range(1, len(date_range)):
        if date_range[i] != date_range[i - 1]:
            n += 1
        day_index[i] = n
    return n, day_index


def run(lib, g, structure, nday, day_index, sparse, nrep=1):
    m = g.mesh
    icfg = np.array([structure, m.nrow, m.ncol, g.nt, int(sparse), nday, nrep], np.int32)
    path = np.asfortranarray(np.asarray(m.path) + 1, dtype=np.int32)
    act = np.asfortranarray(m.active_cell, dtype=np.int32)
    prcp, pet = np.asfortranarray(g.prcp, dtype=np.float32), np.asfortranarray(g.pet, dtype=np.float32)
    day = np.ascontiguousarray(day_index, np.int32)
    ci = np.full((m.nrow, m.ncol), SENTINEL, np.float32, order="F")
    dt, elapsed = C.c_float(g.dt), C.c_double(0.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    lib.ici_run.restype = None
    lib.ici_run(p(icfg), C.byref(dt), p(path), p(act), p(prcp), p(pet), p(day), p(ci), C.byref(elapsed))
    return ci, elapsed.value


def main(timed):
    os.makedirs(iu.DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for name, (structure, start) in RUNS.items():
            g = gu.load(iu.CASES[name])
            nday, day = reference_day_index(start, g.nt, g.dt)
            ci, _ = run(lib, g, structure, nday, day, sparse=False)
            ci_sparse, _ = run(lib, g, structure, nday, day, sparse=True)
            act = np.asarray(g.mesh.active_cell) == 1
            assert np.array_equal(ci, ci_sparse), f"{name}: the reference's dense and sparse branches disagree"
            assert np.all(ci[~act] == SENTINEL) and np.all(ci[act] != SENTINEL), f"{name}: active-cell mask not respected"
            distinct = np.unique(ci[act]).size
            p, e, rows, cols = iu.active_columns(g)
            mine, diff = iu.adjust(p, e, day)
            print(f"{name}: nday {nday}, {int(act.sum())} active cells, {distinct} distinct ci in [{ci[act].min():.1f}, {ci[act].max():.1f}], "
                  f"gaps {int((p < 0).sum() + (e < 0).sum())}, cells with an exact tie of the two best candidates {iu.exact_ties(diff)}, "
                  f"numpy restatement equal on {int(np.sum(mine == ci[rows, cols]))} / {rows.size}")
            if distinct < MIN_DISTINCT:
                print(f"REFUSED: {name} shows {distinct} < {MIN_DISTINCT} distinct capacities: it shows nothing, pick another case")
                return 1
            out = os.path.join(iu.DIR, name + ".npz")
            np.savez_compressed(out, case=iu.CASES[name], structure=structure, start_time=start, nday=nday,
                                day_index=day.astype(np.int32), ci=ci, sentinel=SENTINEL)
            print("wrote", out, os.path.getsize(out), "bytes")
        if timed:
            g = gu.load("gr_a_cance_28x28x1440")
            nday, day = reference_day_index("2014-09-15 00:00", g.nt, g.dt)
            _, sec = run(lib, g, 2, nday, day, sparse=False, nrep=5)
            cells = int((np.asarray(g.mesh.active_cell) == 1).sum())
            print(f"reference routine on gr_a_cance_28x28x1440 (one core, -O2 -ffp-contract=off, best of 5): {sec:.4f} s for {cells} active cells x "
                  f"{g.nt} steps x {iu.candidates().size} candidates = {cells * g.nt / sec:.3e} 49-candidate cell-steps/s")
    return 0


if __name__ == "__main__":
    sys.exit(main("--time" in sys.argv[1:]))
