"""Records tests/golden/signature_cost/: what the compiled reference computes for the signature-based criteria
(mwd_cost.f90:772-970 and SIGNATURE_B / SIGNATURE_D, forward_db.f90:4501-4926), so that tests/test_signature_cost_cpu.py can pin the
numpy restatement (tests/signature_util.py) and tests/test_gpu_signature_cost.py the library where oracle/_ref is absent.

tests/golden/signature_cost_driver.f90 is a bind(C) driver of our own over the UNMODIFIED reference modules; it is compiled here against
the module files and objects oracle/ref/build_ref.sh leaves in oracle/_ref/obj_parity, with the same flags (-O2 -ffp-contract=off), into a
temporary directory: nothing compiled is kept.

  functions.npz            signature, SIGNATURE_B (res_b = 1) and SIGNATURE_D (a recorded random qs_d) on hand-made series of 1 to 200
                           steps, every criterion the reference can evaluate on them (it reads an unassigned num / den on the others);
                           qo, qs and qs_d are 1000 x the raw_* series stored beside them (see function_cases)
  <case>__all.npz          forward, forward_b, forward_d and COMPUTE_JOBS_B of the reference on an existing golden input with
                           jobs_fun = SET_ALL, mean_prcp from tests/golden/mean_forcing/ and a synthetic mask_event
  <case>__median.npz       the same with SET_MEDIAN, negative wgauge (the median over gauges) and optimize_start_step inside the first event

The script refuses to write a fixture in which a requested criterion adds 0 to the cost at every gauge, the Cfp* seeds land on fewer
than two steps, or the tie case's seeds are the ones a stable sort would give.

    python tests/golden/make_signature_cost.py
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
import signature_util as su          # noqa: E402
from smash_amd import synth          # noqa: E402

FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj_parity")
K = np.float32(1e3)
STRUCT = {"gr-a": 1, "gr-b": 2, "gr-c": 3, "gr-d": 4, "vic-a": 5}


OBJ_FAST = os.path.join(ROOT, "oracle", "_ref", "obj_fast")      # the reference as its own makefile builds it (-O3, FMA)


def build(tmp, OBJ=OBJ, opt=("-O2", "-ffp-contract=off")):
    if not os.path.exists(os.path.join(OBJ, "mwd_cost_diff.mod")):
        raise SystemExit(f"{OBJ} lacks mwd_cost_diff.mod: run __graft_entry__.build() where the reference is present")
    os.makedirs(tmp, exist_ok=True)
    flags = ["-cpp", *opt, "-fPIC"]
    obj = os.path.join(tmp, "signature_cost_driver.o")
    subprocess.check_call([FC] + flags + ["-module-dir", tmp, "-I" + OBJ, "-c", os.path.join(HERE, "signature_cost_driver.f90"), "-o", obj])
    lib = os.path.join(tmp, "libsc.so")
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "ref_capi.o"]
    subprocess.check_call([FC, "-shared", "-o", lib, obj] + others)
    return C.CDLL(lib)


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def run_fn(lib, po, qo, qs, mask, qs_d, name):
    n = qo.size
    res, res_d = C.c_float(0), C.c_float(0)
    qs_b = np.zeros(n, np.float32)
    lib.sc_fn.restype = None
    lib.sc_fn(C.c_int(n), C.c_int(su.CODES[name]), p_(po), p_(qo), p_(qs), p_(mask), p_(qs_d), C.byref(res), p_(qs_b), C.byref(res_d))
    return np.float32(res.value), qs_b, np.float32(res_d.value)


# ---- hand-made series ----------------------------------------------------------------------------------------------------------------
def series(rng, n, gaps=0.1):
    """positive series with gaps (negative entries) in qo and po"""
    po = np.where(rng.random(n) < 0.6, 0.0, rng.gamma(1.0, 2.0, n)).astype(np.float32)
    qo = rng.gamma(2.0, 0.5, n).astype(np.float32)
    qs = rng.gamma(2.0, 0.5, n).astype(np.float32)
    qo[rng.random(n) < gaps] = -99.0
    po[rng.random(n) < gaps / 2] = -99.0
    return po, qo, qs


def function_cases():
    rng = np.random.default_rng(20240917)
    cases = {}

    def add(name, po, qo, qs, mask):
        # the routine's qo / qs / qs_d are formed from raw discharges the way compute_jobs forms them for a gauge of unit area on a
        # headwater cell with dt = dx = 1: x 1000 in fp32 (mwd_cost.f90:84-92).  A test that hands the raw series to the library then
        # has the kernels read exactly the series recorded here.
        n = len(qo)
        raw = dict(qobs=su.f32(np.asarray(qo, np.float32) / K), qsim=su.f32(np.asarray(qs, np.float32) / K),
                   qsim_d=(rng.standard_normal(n) / 1e3).astype(np.float32))
        cases[name] = dict(po=su.f32(po), qo=su.f32(raw["qobs"] * K), qs=su.f32(raw["qsim"] * K), mask=np.ascontiguousarray(mask, np.int32),
                           qs_d=su.f32(raw["qsim_d"] * K), raw=raw)

    def blocks(n, spans):
        m = np.zeros(n, np.int32)
        for i, (a, b) in enumerate(spans):
            m[a:b] = i + 1
        return m

    # lengths around the wavefront fold; events that start at step 1 and end at the last step
    for n in (63, 64, 65, 129):
        po, qo, qs = series(rng, n)
        po[0], qo[0], po[n - 1], qo[n - 1] = 1.5, 0.7, 0.5, 0.9
        add(f"len{n}", po, qo, qs, blocks(n, [(0, 9), (20, 41), (n - 12, n)]))
    # n = 1 (a single step) and n = 1 / n = 2 after the percentile's compaction
    add("single", [2.0], [0.5], [0.8], [1])
    po, qo, qs = series(rng, 6, gaps=0.0)
    qo[[0, 1, 3, 4, 5]] = -99.0
    add("compact1", po, qo, qs, blocks(6, [(1, 4)]))
    po, qo, qs = series(rng, 7, gaps=0.0)
    qo[[0, 2, 3, 6]] = -99.0
    qs[1] = -1.0
    po[[4, 5]] = [1.0, 2.0]
    add("compact2", po, qo, qs, blocks(7, [(3, 7)]))
    # frac = (n - 1) p + 1 lands on an integer for every p: 51 valid steps
    po, qo, qs = series(rng, 51, gaps=0.0)
    add("frac_integer", po, qo, qs, blocks(51, [(5, 25), (30, 44)]))
    # the events' corner cases, 200 steps:
    #   1 plain; 2 without any valid step (qo < 0); 3 valid; 4 with sum_po = 0 after a valid one (Erc carries num / den over);
    #   5 with qs = 0 throughout (imax_qs = 0) ; 6 with po = 0 and qo rising (imax_po = 0); 7 split in two runs (its extent is start ..
    #   start + count - 1, which ends inside the gap) ; 8 ends at the last step
    po, qo, qs = series(rng, 200)
    mask = blocks(200, [(3, 20), (25, 33), (40, 66), (70, 84), (90, 101), (105, 118), (125, 133), (170, 200)])
    mask[140:146] = 7
    qo[25:33] = -99.0
    po[70:84] = 0.0
    qs[90:101] = 0.0
    po[105:118] = 0.0
    qo[105:118] = np.linspace(0.2, 1.4, 13, dtype=np.float32)
    po[199], qo[199] = 3.0, 1.1
    add("events200", po, qo, qs, mask)
    # a tie across the Cfp2 position: a run of exact zeros in qs (a cold start), 200 steps
    po, qo, qs = series(rng, 200, gaps=0.05)
    qs[:37] = 0.0
    qs[[60, 61, 150]] = 0.0
    add("tie_zeros", po, qo, qs, blocks(200, [(10, 50), (100, 160)]))
    return cases


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def synthetic_mask(mean_prcp, nt):
    """3 to 5 events per gauge around the wettest steps, numbered in time order, 0 elsewhere"""
    ng = mean_prcp.shape[0]
    mask = np.zeros((ng, nt), np.int32, order="F")
    w = max(2, nt // 60)
    for g in range(ng):
        want, picked = 3 + g % 3, []
        for t in np.argsort(-np.nan_to_num(mean_prcp[g], nan=-1.0), kind="stable"):
            if w + 1 <= t < nt - 3 * w and all(abs(int(t) - q) > 5 * w for q in picked):
                picked.append(int(t))
            if len(picked) == want:
                break
        for i, t in enumerate(sorted(picked)):
            mask[g, t - w:t + 3 * w] = i + 1
    return mask


def elt_possible(g, mean_prcp, qsim):
    """True when some window [a, b) of some gauge gives Elt a term that is not 0: imax_qo - imax_po > 0 and imax_qs != imax_qo"""
    m = g.mesh
    gp = np.asarray(m.gauge_pos).reshape(-1, 2)
    for gi in range(gp.shape[0]):
        qs = su.f32(qsim[gi]) * np.float32(g.dt) / np.float32(m.area[gi]) * np.float32(1e3)
        qo = su.f32(g.qobs[gi]) * np.float32(g.dt) / (np.float32(m.flwacc[gp[gi, 0], gp[gi, 1]]) * np.float32(m.dx) * np.float32(m.dx)) * np.float32(1e3)
        for a in range(g.nt):
            for b in range(a + 1, g.nt + 1):
                r = su._event_fold(su.f32(mean_prcp[gi]), qo, qs, a, b - a)
                if r[6] - r[8] > 0 and r[7] != r[6]:
                    return True
    return False


def pack(fields, names, nrow, ncol):
    a = np.zeros((nrow, ncol, len(names)), np.float32, order="F")
    for i, k in enumerate(names):
        a[:, :, i] = fields[k]
    return a


def run_e2e(lib, g, mean_prcp, mask, jobs, wjobs, wgauge, start, mode, pd=None, sd=None):
    m = g.mesh
    gp = np.asarray(m.gauge_pos).reshape(-1, 2)
    ng, nt = gp.shape[0], g.nt
    icfg = np.array([STRUCT[g.structure], m.nrow, m.ncol, nt, ng, start, len(jobs), mode], np.int32)
    rcfg = np.array([g.dt, m.dx, 1.0], np.float32)
    arr = dict(flw=np.asfortranarray(m.flwdir, dtype=np.int32), acc=np.asfortranarray(m.flwacc, dtype=np.int32),
               path=np.asfortranarray(np.asarray(m.path) + 1, dtype=np.int32), act=np.asfortranarray(m.active_cell, dtype=np.int32),
               gpos=np.asfortranarray(gp + 1, dtype=np.int32), area=su.f32(m.area),
               prcp=np.asfortranarray(g.prcp, dtype=np.float32), pet=np.asfortranarray(g.pet, dtype=np.float32),
               qobs=np.asfortranarray(g.qobs, dtype=np.float32), mp=np.asfortranarray(mean_prcp, dtype=np.float32),
               mask=np.asfortranarray(mask, dtype=np.int32),
               P=pack(g.params, synth.PARAM_NAMES, m.nrow, m.ncol), S=pack(g.states, synth.STATE_NAMES, m.nrow, m.ncol),
               wg=su.f32(wgauge), codes=np.array([su.CODES[j] for j in jobs], np.int32), wj=su.f32(wjobs))
    PD = pd if pd is not None else np.zeros_like(arr["P"])
    SD = sd if sd is not None else np.zeros_like(arr["S"])
    out = dict(qsim=np.zeros((ng, nt), np.float32, order="F"), costs=np.zeros(3, np.float32),
               params_b=np.zeros_like(arr["P"]), states_b=np.zeros_like(arr["S"]),
               qsim_b=np.zeros((ng, nt), np.float32, order="F"), qsim_d=np.zeros((ng, nt), np.float32, order="F"))
    cost_d = C.c_float(0)
    lib.sc_run.restype = None
    lib.sc_run(p_(icfg), p_(rcfg), p_(arr["flw"]), p_(arr["acc"]), p_(arr["path"]), p_(arr["act"]), p_(arr["gpos"]), p_(arr["area"]),
               p_(arr["prcp"]), p_(arr["pet"]), p_(arr["qobs"]), p_(arr["mp"]), p_(arr["mask"]), p_(arr["P"]), p_(arr["S"]), p_(arr["wg"]),
               p_(arr["codes"]), p_(arr["wj"]), p_(PD), p_(SD), p_(out["qsim"]), p_(out["costs"]), p_(out["params_b"]), p_(out["states_b"]),
               p_(out["qsim_b"]), p_(out["qsim_d"]), C.byref(cost_d))
    out["cost_d"] = np.float32(cost_d.value)
    return out


def main():
    os.makedirs(su.DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        # the same driver over the reference built the way its makefile builds it: the distance between the two builds is the
        # reference's own flag-to-flag noise on these very outputs, which the default-build bars of the tests are taken from
        # (tests/golden_util.tol, as tests/golden/make_golden.py records it for the golden fixtures)
        fast = build(os.path.join(tmp, "fast"), OBJ_FAST, ("-O3", "-march=x86-64-v3", "-funroll-loops"))
        # -- function level
        cases = function_cases()
        store = {"cases": np.array(list(cases))}
        for cname, c in cases.items():
            for k in ("po", "qo", "qs", "mask", "qs_d"):
                store[f"{cname}__{k}"] = c[k]
            for k, v in c["raw"].items():
                store[f"{cname}__raw_{k}"] = v
            done = []
            for nm in su.NAMES:
                if su.refused(c["po"], c["qo"], c["mask"], nm):
                    continue
                res, qs_b, res_d = run_fn(lib, c["po"], c["qo"], c["qs"], c["mask"], c["qs_d"], nm)
                store[f"{cname}__{nm}__res"], store[f"{cname}__{nm}__qs_b"], store[f"{cname}__{nm}__res_d"] = res, qs_b, res_d
                mine = su._walk(c["po"], c["qo"], c["qs"], c["mask"], nm, c["qs_d"])
                ok = su.same_bits(mine[0], res) and su.same_bits(mine[1], qs_b) and su.same_bits(mine[2], res_d)
                done.append(nm + ("" if ok else "(restatement differs)"))
            print(f"{cname}: n = {c['qo'].size}, recorded {done}")
        c = cases["tie_zeros"]
        for nm in ("Cfp2",):
            got = tuple(int(k) for k in np.flatnonzero(store[f"tie_zeros__{nm}__qs_b"]))
            stable = tuple(sorted(k for k in su.stable_points(c["qo"], c["qs"], su.PCT[nm]) if k >= 0))
            print(f"tie_zeros {nm}: the reference seeds steps {got}, a stable sort would seed {stable}")
            if got == stable or not all(c["qs"][k] == 0 for k in got):
                print("REFUSED: the tie case does not tell the heap sort from a stable sort; change the series")
                return 1
        out = os.path.join(su.DIR, "functions.npz")
        np.savez_compressed(out, **store)
        print("wrote", out, os.path.getsize(out), "bytes")
        # -- end to end
        rng = np.random.default_rng(7)
        for case in su.E2E_CASES:
            g = gu.load(case)
            m = g.mesh
            ng, nt = np.asarray(m.gauge_pos).reshape(-1, 2).shape[0], g.nt
            mean_prcp = np.load(os.path.join(HERE, "mean_forcing", case + ".npz"))["mean_prcp"]
            mask = synthetic_mask(mean_prcp, nt)
            first = np.flatnonzero(mask[0] == 1)
            variants = {"all": (su.SET_ALL, [0.3, 0.05, 0.1, 0.15, 0.1, 0.1, 0.12, 0.08], np.array([0.5, 0.3, 0.2], np.float32)[:ng], 1),
                        "median": (su.SET_MEDIAN, [0.5, 0.2, 0.3], np.full(ng, -1.0, np.float32), int(first[len(first) // 2]) + 1)}
            names_p, names_s = gu.STRUCT_PARAMS[g.structure], gu.STRUCT_STATES[g.structure]
            for tag, (jobs, wjobs, wgauge, start) in variants.items():
                fwd = run_e2e(lib, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 0)
                adj = run_e2e(lib, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 1)
                # the direction of the tangent: 1 % of every field, signed like the gradient (as tests/golden/make_golden.py does: a
                # random direction makes cost_d a cancelling sum)
                pd = np.zeros((m.nrow, m.ncol, len(synth.PARAM_NAMES)), np.float32, order="F")
                sd = np.zeros((m.nrow, m.ncol, len(synth.STATE_NAMES)), np.float32, order="F")
                for k in names_p:
                    i = synth.PARAM_NAMES.index(k)
                    pd[:, :, i] = 0.01 * np.maximum(np.abs(g.params[k]), 1e-3) * np.sign(adj["params_b"][:, :, i])
                for k in names_s:
                    i = synth.STATE_NAMES.index(k)
                    sd[:, :, i] = 0.01 * np.maximum(np.abs(g.states[k]), 1e-3) * np.sign(adj["states_b"][:, :, i])
                tan = run_e2e(lib, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 3, pd, sd)
                assert su.same_bits(fwd["qsim"], adj["qsim"]) and su.same_bits(fwd["costs"], adj["costs"])
                # every criterion must add to the cost somewhere: the reference run with that criterion alone
                zero_everywhere = []
                for j in jobs:
                    alone = run_e2e(lib, g, mean_prcp, mask, (j,), [1.0], np.abs(wgauge) / np.abs(wgauge).sum(), start, 0)["costs"][0]
                    print(f"  {case} {tag}: {j} alone costs {alone:.6g}")
                    if not abs(alone) > 0:
                        if j == "Elt" and not elt_possible(g, mean_prcp, fwd["qsim"]):
                            # no mask can help: whatever the window, the simulated and the observed peak fall on the same step wherever
                            # the observed one follows the rain's.  Recorded as it is, and said in the fixture.
                            print(f"  {case} {tag}: Elt is 0 for EVERY window of every gauge of this input (exhaustive search), not only for this mask")
                            zero_everywhere.append(j)
                            continue
                        print(f"REFUSED: {j} adds nothing to the cost of {case} ({tag}); change the mask or the case")
                        return 1
                pct = [j for j in jobs if j.startswith("Cfp")]
                if pct:
                    qb = run_e2e(lib, g, mean_prcp, mask, pct, [1.0] * len(pct), np.abs(wgauge) / np.abs(wgauge).sum(), start, 0)["qsim_b"]
                    steps = np.unique(np.nonzero(qb)[1])
                    print(f"  {case} {tag}: the Cfp* seeds land on steps {steps.tolist()}")
                    if steps.size < 2:
                        print("REFUSED: the Cfp* seeds land on fewer than two steps")
                        return 1
                f_fwd = run_e2e(fast, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 0)
                f_adj = run_e2e(fast, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 1)
                f_tan = run_e2e(fast, g, mean_prcp, mask, jobs, wjobs, wgauge, start, 3, pd, sd)
                noise = dict(noise_cost=np.float64(abs(float(f_fwd["costs"][0]) - float(fwd["costs"][0])) / abs(float(fwd["costs"][0]))),
                             noise_cost_d=np.float64(abs(float(f_tan["cost_d"]) - float(tan["cost_d"])) / abs(float(tan["cost_d"]))),
                             noise_qsim=np.array([gu.rel_l2(f_fwd["qsim"][i], fwd["qsim"][i]) for i in range(ng)]),
                             noise_qsim_d=np.array([gu.rel_l2(f_tan["qsim_d"][i], tan["qsim_d"][i]) for i in range(ng)]))
                for k in names_p:
                    i = synth.PARAM_NAMES.index(k)
                    noise["noise_b_" + k] = np.float64(gu.rel_l2(f_adj["params_b"][:, :, i], adj["params_b"][:, :, i]))
                for k in names_s:
                    i = synth.STATE_NAMES.index(k)
                    noise["noise_b_" + k] = np.float64(gu.rel_l2(f_adj["states_b"][:, :, i], adj["states_b"][:, :, i]))
                print(f"  {case} {tag}: the reference's own two builds differ by", {k: float(np.max(v)) for k, v in noise.items()})
                rec = dict(case=case, **noise, jobs_fun=np.array(jobs), wjobs_fun=su.f32(wjobs), wgauge=wgauge, optimize_start_step=start,
                           mask_event=mask, zero_everywhere=np.array(zero_everywhere, dtype="U8"), cost=fwd["costs"][0], qsim=fwd["qsim"], qsim_b=fwd["qsim_b"], cost_d=tan["cost_d"], qsim_d=tan["qsim_d"])
                for k in names_p:
                    i = synth.PARAM_NAMES.index(k)
                    rec["b_" + k], rec["d_" + k] = adj["params_b"][:, :, i], pd[:, :, i]
                for k in names_s:
                    i = synth.STATE_NAMES.index(k)
                    rec["b_" + k], rec["d_" + k] = adj["states_b"][:, :, i], sd[:, :, i]
                out = os.path.join(su.DIR, f"{case}__{tag}.npz")
                np.savez_compressed(out, **rec)
                print(f"{case} {tag}: cost {fwd['costs'][0]:.7g}, cost_d {tan['cost_d']:.7g}, start step {start}; wrote {out} {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
