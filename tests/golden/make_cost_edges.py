"""Records tests/golden/cost_edges/cost_edges.npz: what the compiled reference computes for the gauge cost stage (compute_jobs,
COMPUTE_JOBS_B, COMPUTE_JOBS_D: mwd_cost.f90:37-156, forward_db.f90:2445-2715) on the prescribed series of tests/cost_edge_cases.py,
so that tests/test_cost_edges_cpu.py can pin the numpy restatement and tests/test_gpu_cost_edges.py the library where oracle/_ref is
absent.

tests/golden/cost_edges_driver.f90 is a bind(C) driver of our own over the UNMODIFIED reference modules; it is compiled here against
the module files and objects oracle/ref/build_ref.sh leaves in oracle/_ref/obj_parity, with the same flags (-O2 -ffp-contract=off),
into a temporary directory: nothing compiled is kept.

Per case: the inputs, jobs, jobs_d, output_b%qsim for jobs_b = 1 and for jobs_b = 2.5, and per criterion of the case whether the
reference's value of that criterion alone is finite.  The empty-gauge cases are not recorded: the reference reads an unassigned
local there.

The script refuses to write a fixture in which a case does not reach what its name claims (cost_edge_cases' claims): the count n of
each gauge, qs == qo / var_x = 0 / var_y = 0 where claimed, the median's size, branch and index, that a tie at the interpolation points hands the seed to
a gauge a stable sort would NOT choose, that every criterion that is finite leaves a non-zero seed when it
runs alone (but where qs == qo, where the derivatives are 0 or guarded), and that at least three quarters of the (case, criterion) pairs are finite.

    python tests/golden/make_cost_edges.py
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

import cost_edge_cases as ce         # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj_parity")
F32 = np.float32


def build(tmp):
    if not os.path.exists(os.path.join(OBJ, "mwd_cost_diff.mod")):
        raise SystemExit(f"{OBJ} lacks mwd_cost_diff.mod: run __graft_entry__.build() where the reference is present")
    obj = os.path.join(tmp, "cost_edges_driver.o")
    subprocess.check_call([FC, "-cpp", "-O2", "-ffp-contract=off", "-fPIC", "-module-dir", tmp, "-I" + OBJ, "-c",
                           os.path.join(HERE, "cost_edges_driver.f90"), "-o", obj])
    lib = os.path.join(tmp, "libce.so")
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "ref_capi.o"]
    subprocess.check_call([FC, "-shared", "-o", lib, obj] + others)
    return C.CDLL(lib)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def run(lib, c, jobs=None, wjobs=None):
    """the reference on case c (with other criteria when given): dict(jobs, jobs_d, qsim_b1, qsim_b2)"""
    m = ce.base_mesh()
    jobs = c["jobs"] if jobs is None else jobs
    wjobs = c["wjobs"] if wjobs is None else np.array(wjobs, F32)
    ng, nt = c["ng"], c["nt"]
    icfg = np.array([m.nrow, m.ncol, nt, ng, c["start"], len(jobs)], np.int32)
    rcfg = np.array([ce.DT, ce.DX, ce.JOBS_B[0], ce.JOBS_B[1]], F32)
    a = dict(acc=np.asfortranarray(m.flwacc, dtype=np.int32), gp=np.asfortranarray(c["gauge_pos"] + 1, dtype=np.int32),
             area=np.ascontiguousarray(c["area"], F32), codes=np.array([ce.CODES[j] for j in jobs], np.int32), wg=np.ascontiguousarray(c["wgauge"], F32))
    res = np.zeros(3, F32)
    b1, b2 = np.zeros((ng, nt), F32, order="F"), np.zeros((ng, nt), F32, order="F")
    lib.ce_run.restype = None
    lib.ce_run(p_(icfg), p_(rcfg), p_(a["acc"]), p_(a["gp"]), p_(a["area"]), p_(c["qobs"]), p_(c["qsim"]), p_(c["qsim_d"]), p_(a["wg"]),
               p_(a["codes"]), p_(wjobs), p_(res), p_(b1), p_(b2))
    return dict(jobs=res[0], jobs_d=res[1], qsim_b1=b1, qsim_b2=b2)


def check_claims(c, ref, mine, finite):
    """what the case's name promises, on the restatement's diagnostics (which the recorded outputs pin) and the reference's seeds"""
    cl, name = c["claims"], c["name"]
    why = []
    if list(mine["n"]) != list(cl["n"]):
        why.append(f"n per gauge {list(mine['n'])}, claimed {cl['n']}")
    qo, qs, _ = ce.normalised(c)
    s0 = c["start"] - 1
    cnt = qo[:, s0:] >= 0
    if cl.get("equal") and not np.array_equal(qo[:, s0:][cnt], qs[:, s0:][cnt]):
        why.append("qs != qo on a counted step")
    for key, arr in (("var_x0", qo), ("var_y0", qs)):
        if cl.get(key) and not all(np.unique(arr[g, s0:][cnt[g]]).size == 1 for g in range(c["ng"])):
            why.append(key + ": the series is not constant")
    if cl.get("var_x0") and "nse" in c["jobs"] and np.isfinite(run_alone[name]["nse"]):
        why.append("constant observations but nse is finite: den != 0")
    if "median" in cl:
        m = cl["median"]
        want = ("interp", int((m - 1) * 0.5 + 1)) if m > 1 else (None, None)
        if len(mine["perm"] or []) != m or (mine["branch"], mine["k"]) != want:
            why.append(f"median over {len(mine['perm'] or [])} ({mine['branch']}, k = {mine['k']}), claimed {m} {want}")
        if not np.isfinite(mine["gauge_jobs"][c["wgauge"] < 0]).all():
            why.append("a NaN or Inf in a median case")
        seeded_ref = tuple(int(g) for g in np.flatnonzero(np.any(ref["qsim_b1"] != 0, axis=1)))
        if seeded_ref != tuple(sorted(mine["seeded"])):
            why.append(f"the reference seeds gauges {seeded_ref}, the restatement {mine['seeded']}")
        if "tie" in cl:
            tied, pts, seeded, stable = ce.tie_report(c, mine)
            if not tied or bool(set(pts) & set(tied)) != (cl["tie"] == "at"):
                why.append(f"tie {tied} against the interpolation points {pts}: claimed {cl['tie']}")
            print(f"  {name}: sorted gauges {mine['perm']}, tied {tied}, the reference seeds {seeded_ref}; a stable sort would seed {stable}")
            if cl["tie"] == "at" and seeded_ref == stable:
                why.append("the tie case does not tell the heap sort from a stable sort")
    # every criterion that is finite gives a seed somewhere when it runs alone.  Waived where qs == qo on every counted step: the
    # derivative of nse, se and logarithmic is 0 there and those of rmse and kge are the guarded ones, which is what the case is for.
    for j, ok in finite.items():
        b = seeds_alone[name][j]
        if ok and not cl.get("equal") and not np.any(b[np.isfinite(b)]):
            why.append(f"{j} alone is finite but leaves no seed")
    return why


run_alone, seeds_alone = {}, {}


def main():
    os.makedirs(ce.DIR, exist_ok=True)
    cases = ce.cases()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        store = {"cases": np.array(list(cases))}
        pairs = fin = 0
        refused = []
        for name, c in cases.items():
            ref = run(lib, c)
            crits = sorted(set(c["jobs"]), key=ce.CRIT.index)
            alone = {j: run(lib, c, (j,), (1.0,)) for j in crits}
            run_alone[name], seeds_alone[name] = {j: a["jobs"] for j, a in alone.items()}, {j: a["qsim_b1"] for j, a in alone.items()}
            finite = {j: bool(np.isfinite(v)) for j, v in run_alone[name].items()}
            pairs, fin = pairs + len(finite), fin + sum(finite.values())
            mine = ce.restate(c, jobs_b=ce.JOBS_B[0])
            mine2 = ce.restate(c, jobs_b=ce.JOBS_B[1])
            ok = (ce.same_bits(mine["jobs"], ref["jobs"]) and ce.same_bits(mine["jobs_d"], ref["jobs_d"])
                  and ce.same_bits(mine["qsim_b"], ref["qsim_b1"]) and ce.same_bits(mine2["qsim_b"], ref["qsim_b2"]))
            why = check_claims(c, ref, mine, finite)
            print(f"{name}: ng {c['ng']} nt {c['nt']} start {c['start']} {'+'.join(c['jobs'])}: jobs {ref['jobs']!r} jobs_d {ref['jobs_d']!r} "
                  f"seeds {int(np.count_nonzero(ref['qsim_b1']))} not finite {[j for j, f in finite.items() if not f]}"
                  + ("" if ok else "  (RESTATEMENT DIFFERS)") + ("".join("\n  REFUSED: " + w for w in why)))
            refused += [name] * bool(why)
            for k in ce.INPUTS:
                store[f"{name}__{k}"] = c[k]
            store[f"{name}__jobs_fun"], store[f"{name}__start"] = np.array(c["jobs"]), np.int32(c["start"])
            store[f"{name}__finite"] = np.array([finite[j] for j in crits])
            for k, v in ref.items():
                store[f"{name}__{k}"] = v
        print(f"{fin} of {pairs} (case, criterion) pairs are finite in the reference")
        if 4 * fin < 3 * pairs:
            print("REFUSED: fewer than three quarters of the (case, criterion) pairs are finite")
            refused.append("finite")
        if refused:
            print("nothing written:", refused)
            return 1
        np.savez_compressed(ce.FIXTURE, **store)
        print("wrote", ce.FIXTURE, os.path.getsize(ce.FIXTURE), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
