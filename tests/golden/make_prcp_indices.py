"""Records tests/golden/prcp_indices/<case>.npz: the precipitation indices the compiled reference forms
(mw_forcing_statistic::compute_prcp_indices, smash/solver/routine/mw_forcing_statistic.f90:77-220) on the rain of existing fixtures,
so that tests/test_prcp_indices_cpu.py can pin the numpy restatement (tests/prcp_indices_util.py) and tests/test_gpu_prcp_indices.py
the library against the reference where oracle/_ref is absent.

oracle/ref/ref_capi.f90 has no entry for this routine; tests/golden/prcp_indices_driver.f90 is a bind(C) driver of our own.  It is
compiled here against the module files and objects oracle/ref/build_ref.sh leaves in oracle/_ref/obj_parity, with the same flags
(-O2 -ffp-contract=off), into a temporary directory: nothing compiled is kept.

Stored per fixture: flwdst (nrow, ncol), the plane the run was given (smash_amd.synth.flow_distance of the case's mesh: the golden cases
carry none), prcp_indices (4, ng, nt) as the routine left it from a prefill of -7, and the case's name.  The forcing is the golden
case's and is not stored again.  Every case is also run with sparse storage (the reference's other branch must agree bit for bit,
NaN = NaN).  The script REFUSES to write unless
  (a) every case has at least 64 (gauge, step) pairs written and at least 8 left at the sentinel (gr_b_16x16x96_nse_gaps has rain on
      14 steps only, 40 pairs: it is let off the 64, see FEW_WRITTEN in tests/prcp_indices_util.py, and recorded a second time as
      the __wet variant, which meets every condition);
  (b) every case has at least 8 written pairs on which the result differs from the same formulas fed with fp64 sums rounded once;
  (c) over the cases with a gauge whose row differs from its column, at least 8 pairs change when pwf(1) is read from
      (row, col) instead of the reference's (row, row);
  (d) at least one case has an active cell outside a catchment inside one of that gauge's distance bins.

    python tests/golden/make_prcp_indices.py
"""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, ROOT)

import golden_util as gu             # noqa: E402
import prcp_indices_util as pu       # noqa: E402
from smash_amd import synth          # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj_parity")
MIN_WRITTEN, MIN_LEFT, MIN_SEQUENTIAL, MIN_ROWROW = 64, 8, 8, 8


def build(tmp):
    """the driver + the reference's objects -> tmp/libpi.so"""
    if not os.path.exists(os.path.join(OBJ, "mw_forcing_statistic.mod")):
        raise SystemExit(f"{OBJ} lacks mw_forcing_statistic.mod: run __graft_entry__.build() where the reference is present")
    flags = ["-cpp", "-O2", "-ffp-contract=off", "-fPIC"]
    obj = os.path.join(tmp, "prcp_indices_driver.o")
    subprocess.check_call([FC] + flags + ["-module-dir", tmp, "-I" + OBJ, "-c", os.path.join(HERE, "prcp_indices_driver.f90"), "-o", obj])
    lib = os.path.join(tmp, "libpi.so")
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "ref_capi.o"]
    subprocess.check_call([FC, "-shared", "-o", lib, obj] + others)
    return C.CDLL(lib)


def run(lib, g, prcp, flwdst, sparse):
    m = g.mesh
    gp = np.asarray(m.gauge_pos).reshape(-1, 2)
    ng = gp.shape[0]
    icfg = np.array([m.nrow, m.ncol, g.nt, ng, int(sparse)], np.int32)
    flw = np.asfortranarray(m.flwdir, dtype=np.int32)
    path = np.asfortranarray(np.asarray(m.path) + 1, dtype=np.int32)
    act = np.asfortranarray(m.active_cell, dtype=np.int32)
    gpos = np.asfortranarray(gp + 1, dtype=np.int32)
    dst = np.asfortranarray(flwdst, dtype=np.float32)
    prcp = np.asfortranarray(prcp, dtype=np.float32)
    out = pu.sentinels(ng, g.nt)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    lib.pi_run.restype = None
    lib.pi_run(p(icfg), p(flw), p(path), p(act), p(gpos), p(dst), p(prcp), p(out))
    return out


def pairs_differing(a, b):
    """(gauge, step) pairs on which any of the four entries differs"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.any((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32))), axis=0).sum())


def main():
    os.makedirs(pu.DIR, exist_ok=True)
    todo, rowrow, outside = [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for name, case in pu.CASES.items():
            g = gu.load(case)
            m = g.mesh
            prcp = pu.rain(name, g.prcp)
            act = np.asarray(m.active_cell) == 1
            gp = np.asarray(m.gauge_pos).reshape(-1, 2)
            flwdst = synth.flow_distance(m.flwdir, m.active_cell, m.dx)
            tabs = pu.gauge_tables(m.flwdir, m.gauge_pos, flwdst)
            for T in tabs:
                assert np.all(act[T["rows"], T["cols"]]), f"{name}: a catchment leaves the active cells"
                assert T["row"] < m.ncol and act[T["row"], T["row"]], f"{name}: the (row, row) cell of a gauge is not active"
                inside = np.zeros(act.shape, bool)
                inside[T["rows"], T["cols"]] = True
                for br, bc in T["bins"]:
                    assert np.all(act[br, bc]), f"{name}: a distance bin holds an inactive cell (the sparse branch is undefined there)"
                    outside += int(np.count_nonzero(~inside[br, bc]))
            ref = run(lib, g, prcp, flwdst, sparse=False)
            assert pu.same_bits(ref, run(lib, g, prcp, flwdst, sparse=True)), f"{name}: the reference's dense and sparse branches disagree"
            mine = pu.sentinels(m.ng, g.nt)
            written = pu.prcp_indices(m.flwdir, m.gauge_pos, flwdst, prcp, mine)
            wide = pu.sentinels(m.ng, g.nt)
            pu.prcp_indices(m.flwdir, m.gauge_pos, flwdst, prcp, wide, wide=True)
            left = np.all(ref == pu.SENTINEL, axis=0)
            nwritten, nleft, nseq = int((~left).sum()), int(left.sum()), pairs_differing(ref[:, ~left], wide[:, ~left])
            ncol = 0
            if np.any(gp[:, 0] != gp[:, 1]):
                other = pu.sentinels(m.ng, g.nt)
                pu.prcp_indices(m.flwdir, m.gauge_pos, flwdst, prcp, other, gauge_col=True)
                ncol = pairs_differing(mine, other)
                rowrow += ncol
            print(f"{name}: catchments of {[T['rows'].size for T in tabs]} cells, gauges {gp.tolist()}, {g.nt} steps: {nwritten} pairs written, {nleft} left, "
                  f"NaN entries {int(np.isnan(ref).sum())}, numpy restatement differs on {pu.count_differing(ref, mine)} of {ref.size} entries "
                  f"(written sets equal: {bool(np.array_equal(written, ~left))}), fp64 sums rounded once differ on {nseq} pairs, "
                  f"(row, col) for (row, row) changes {ncol} pairs")
            few = pu.FEW_WRITTEN.get(name)
            if few is not None:
                assert nwritten == few < MIN_WRITTEN, f"{name}: {nwritten} pairs written, the note in prcp_indices_util.py says {few}"
            if (few is None and nwritten < MIN_WRITTEN) or nleft < MIN_LEFT or nseq < MIN_SEQUENTIAL:
                print(f"REFUSED: {name} does not meet (a) / (b): pick another case")
                return 1
            todo.append((name, flwdst, ref))
        if rowrow < MIN_ROWROW:
            print(f"REFUSED: (c) the row / column quirk shows on {rowrow} < {MIN_ROWROW} pairs")
            return 1
        if outside < 1:
            print("REFUSED: (d) no case has a cell outside a catchment inside a distance bin")
            return 1
        print(f"(c) {rowrow} pairs tell (row, row) from (row, col); (d) {outside} bin cells lie outside their gauge's catchment")
        for name, flwdst, ref in todo:
            out = os.path.join(pu.DIR, name + ".npz")
            np.savez_compressed(out, case=pu.CASES[name], flwdst=flwdst, prcp_indices=ref)
            print("wrote", out, os.path.getsize(out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
