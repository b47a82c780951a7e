"""The gauge cost stage (compute_jobs / COMPUTE_JOBS_B / COMPUTE_JOBS_D: smash_amd/csrc/sx_cost.h) at its edges: the cases of
tests/test_cost_edges_cpu.py, tests/test_gpu_cost_edges.py and the recipe tests/golden/make_cost_edges.py.  A plain helper module
like jreg_cases.py.

A case is a prescribed triple (qobs, qsim, qsim_d) of shape (ng, nt) with gauge weights, criteria and a start step, on the 12 x 12 mesh
of the golden input gr_a_12x12x48_nse with dt = 3600 s and dx = 500 m.  The gauges sit on distinct active cells (smashx_jobs_of_qsim
refuses shared ones) in the order of falling flow accumulation, so their flwacc differ, and every gauge has an area of its own: the
two normalisations qs = q dt / area 1e3 and qo = qobs dt / (flwacc dx dx) 1e3 are under test with the sums.  Two kinds of gauge
depart from that on purpose: "matched" gauges have area = flwacc dx dx exactly, so that qsim == qobs gives qs == qo bit for bit, and
"twin" gauges sit on headwater cells (flwacc = 1) with one common area and one common series, so that their gauge_jobs are EQUAL
bits with non-zero seeds -- which of them the median's unstable heap sort hands the seed to is the point of the tie cases.
In front of the start step every series holds junk: large values and missing flags that would change every sum if they were read.

CASES (built once by cases()) holds the recorded cases, for which tests/golden/cost_edges/cost_edges.npz has what the compiled
reference computes, and EMPTY the cases with a gauge that has a non-zero weight and no observation from the start step on.  There
is no reference for those: the compiled reference reads a local it never assigned; the library and the oracle
count such a gauge exactly as if its weight were 0, and the tests hold them to that.

NaN is kept out of every case with a median (a negative weight): an ordered comparison with a NaN operand may be compiled either way
round in the reference's heap sort, so where a NaN gauge_jobs would land is not defined by its source.  Elsewhere non-finite results
are expected (one counted step, constant observations) and are not left out: the comparison is "same fp32 bits, or both NaN".

restate(case, dtype) is a numpy restatement of compute_jobs, COMPUTE_JOBS_B and COMPUTE_JOBS_D for the six classic criteria,
sequential in time like the reference: with dtype = float32 it must reproduce the fixture bit for bit (logf is glibc's, through
ctypes, as in the compiled reference); with float64 it is the truth the default build's logarithmic is judged against."""
from __future__ import annotations

import ctypes
import ctypes.util
import math
import os

import numpy as np

import golden_util as gu

F32 = np.float32
DT, DX = 3600.0, 500.0
BASE = "gr_a_12x12x48_nse"
CRIT = ("nse", "kge", "kge2", "se", "rmse", "logarithmic")
CODES = {k: i + 1 for i, k in enumerate(CRIT)}
DIR = os.path.join(gu.GOLDEN_DIR, "cost_edges")
FIXTURE = os.path.join(DIR, "cost_edges.npz")
JOBS_B = (1.0, 2.5)                  # the two seeds COMPUTE_JOBS_B is recorded with: a seed scaled twice shows in the second
MISSING = F32(-99.0)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def same_bits(a, b):
    """same fp32 bits, or both NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the mesh and the gauges -------------------------------------------------------------------------------------------------------------
_mesh = None


def base_mesh():
    global _mesh
    if _mesh is None:
        _mesh = gu.load(BASE).mesh
    return _mesh


def layout(ng, matched=(), twins=()):
    """(gauge_pos (ng, 2) 0-based, flwacc (ng,), area (ng,) float32): gauge g on the g-th active cell in the order of falling flow
    accumulation; the twins on the LAST cells of that order, which are headwater cells"""
    m = base_mesh()
    fa, act = np.asarray(m.flwacc), np.asarray(m.active_cell)
    cells = sorted(((int(r), int(c)) for r, c in zip(*np.nonzero(act == 1))), key=lambda rc: (-int(fa[rc]), rc))
    assert ng <= len(cells)
    gp, acc, area = np.zeros((ng, 2), np.int32), np.zeros(ng, np.int32), np.zeros(ng, F32)
    front = 0
    for g in range(ng):
        if g in twins:
            rc = cells[len(cells) - 1 - list(twins).index(g)]
            assert fa[rc] == 1
        else:
            rc = cells[front]
            front += 1
        gp[g], acc[g] = rc, fa[rc]
        cell = F32(acc[g]) * F32(DX) * F32(DX)
        area[g] = F32(DX * DX * 1.25) if g in twins else cell if g in matched else cell * F32(0.75 + 0.0625 * (g % 9))
    assert len({tuple(p) for p in gp}) == ng
    return np.asfortranarray(gp), acc, area


# ---- the series ----------------------------------------------------------------------------------------------------------------------------
def _raw(lay, qo, qs, qs_d):
    """raw discharges whose normalised values are near qo, qs, qs_d"""
    _, acc, area = lay
    ko = (acc.astype(np.float64) * DX * DX / (DT * 1e3))[:, None]
    ks = (area.astype(np.float64) / (DT * 1e3))[:, None]
    return (np.asfortranarray((qo * ko).astype(F32)), np.asfortranarray((qs * ks).astype(F32)), np.asfortranarray((qs_d * ks).astype(F32)))


def _series(rng, lay, nt, s0):
    ng = lay[1].size
    qo = 0.2 + 2.0 * rng.random((ng, nt))
    qs = qo * (0.7 + 0.6 * rng.random((ng, nt)))
    qs_d = rng.random((ng, nt)) - 0.4
    qobs, qsim, qsim_d = _raw(lay, qo, qs, qs_d)
    # junk in front of the start step: large values with every third observation missing
    qobs[:, :s0] = (F32(40.0) * qobs[:, :s0]).astype(F32)
    qobs[:, :s0:3] = MISSING
    qsim[:, :s0] = (F32(-25.0) * qsim[:, :s0]).astype(F32)
    qsim_d[:, :s0] = F32(3.0)
    return qobs, qsim, qsim_d


def _case(name, ng, nt, s0, jobs, wjobs, wgauge, seed, matched=(), twins=(), edit=None, claims=None):
    lay = layout(ng, matched, twins)
    rng = np.random.default_rng([20241021, seed])
    qobs, qsim, qsim_d = _series(rng, lay, nt, s0)
    for g in list(twins)[1:]:
        qobs[g], qsim[g], qsim_d[g] = qobs[twins[0]], qsim[twins[0]], qsim_d[twins[0]]
    c = dict(name=name, ng=ng, nt=nt, start=s0 + 1, jobs=tuple(jobs), wjobs=np.array(wjobs, F32), wgauge=np.array(wgauge, F32),
             gauge_pos=lay[0], flwacc=lay[1], area=lay[2], qobs=qobs, qsim=qsim, qsim_d=qsim_d, claims=dict(claims or {}))
    assert len(c["jobs"]) == c["wjobs"].size <= 8 and c["wgauge"].size == ng and 0 <= s0 < nt
    if edit:
        edit(c, rng)
    for k in ("qobs", "qsim", "qsim_d"):
        c[k] = np.asfortranarray(c[k], F32)
    return c


def normalised(c, dtype=F32):
    """(qo, qs, qs_d) of the whole series as compute_jobs forms them (mwd_cost.f90:84-92, forward_db.f90:2500-2510), in dtype"""
    T = dtype
    dt, dx, k = T(DT), T(DX), T(1e3)
    qo = np.empty((c["ng"], c["nt"]), T); qs = np.empty_like(qo); qd = np.empty_like(qo)
    with np.errstate(all="ignore"):
        for g in range(c["ng"]):
            a, f = T(c["area"][g]), T(F32(c["flwacc"][g]))
            qs[g] = c["qsim"][g].astype(T) * dt / a * k
            qo[g] = c["qobs"][g].astype(T) * dt / (f * dx * dx) * k
            qd[g] = k * dt * c["qsim_d"][g].astype(T) / a
    return qo, qs, qd


def _set_qo(c, g, t, want):
    """qobs[g, t] := an fp32 value whose normalised qo is exactly want (fp32); searched among the neighbours of the quotient"""
    f = float(c["flwacc"][g]) * DX * DX / (DT * 1e3)
    q = F32(want * f)
    for _ in range(64):
        got = F32(F32(F32(q * F32(DT)) / F32(F32(F32(c["flwacc"][g]) * F32(DX)) * F32(DX))) * F32(1e3))
        if got == F32(want):
            c["qobs"][g, t] = q
            return
        q = np.nextafter(q, F32(np.inf) if got < want else F32(-np.inf))
    raise AssertionError(f"no fp32 qobs gives qo = {want} at gauge {g}")


def _set_qs(c, g, t, want):
    f = float(c["area"][g]) / (DT * 1e3)
    q = F32(want * f)
    for _ in range(64):
        got = F32(F32(F32(q * F32(DT)) / c["area"][g]) * F32(1e3))
        if got == F32(want):
            c["qsim"][g, t] = q
            return
        q = np.nextafter(q, F32(np.inf) if got < want else F32(-np.inf))
    raise AssertionError(f"no fp32 qsim gives qs = {want} at gauge {g}")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def _log(T, v):
    return F32(_libm.logf(float(v))) if T is F32 else T(math.log(v))


def _sums(T, x, y, yd):
    z = T(0)
    S = dict(n=0, sx=z, sy=z, sxx=z, syy=z, sxy=z, se=z, lg=z, sy_d=z, syy_d=z, sxy_d=z, se_d=z, lg_d=z)
    two = T(2)
    for i in range(x.size):
        xi, yi, di = x[i], y[i], yd[i]
        if xi >= 0:
            S["n"] += 1
            S["sx"] = S["sx"] + xi; S["sy"] = S["sy"] + yi
            S["sxx"] = S["sxx"] + xi * xi; S["syy"] = S["syy"] + yi * yi; S["sxy"] = S["sxy"] + xi * yi
            S["se"] = S["se"] + (xi - yi) * (xi - yi)
            S["sy_d"] = S["sy_d"] + di; S["syy_d"] = S["syy_d"] + two * yi * di; S["sxy_d"] = S["sxy_d"] + xi * di
            S["se_d"] = S["se_d"] - two * (xi - yi) * di
        if xi > 0 and yi > 0:
            a_d, a = di / xi, yi / xi
            t = _log(T, a)
            S["lg"] = S["lg"] + xi * t * t                       # mwd_cost.f90:558-592: (x log) log
            S["lg_d"] = S["lg_d"] + xi * (t * a_d / a + t * a_d / a)
    return S


def _kge(T, S):
    n = T(S["n"])
    k = dict(mean_x=S["sx"] / n, mean_y=S["sy"] / n)
    k["var_x"] = S["sxx"] / n - k["mean_x"] * k["mean_x"]
    k["var_y"] = S["syy"] / n - k["mean_y"] * k["mean_y"]
    k["cov"] = S["sxy"] / n - k["mean_x"] * k["mean_y"]
    k["r"] = (k["cov"] / np.sqrt(k["var_x"])) / np.sqrt(k["var_y"])
    k["a"] = np.sqrt(k["var_y"]) / np.sqrt(k["var_x"])
    k["b"] = k["mean_y"] / k["mean_x"]
    one = T(1)
    k["arg1"] = (k["r"] - one) * (k["r"] - one) + (k["b"] - one) * (k["b"] - one) + (k["a"] - one) * (k["a"] - one)
    return k


def _value(T, S, fun):
    n = T(S["n"])
    if fun == "nse":
        mean_x = S["sx"] / n
        return (S["sxx"] - T(2) * S["sxy"] + S["syy"]) / (S["sxx"] - n * mean_x * mean_x)
    if fun in ("kge", "kge2"):
        v = np.sqrt(_kge(T, S)["arg1"])
        return v if fun == "kge" else v * v
    if fun == "se":
        return S["se"]
    if fun == "rmse":
        return np.sqrt(S["se"] / n)
    return S["lg"]


def _tangent(T, S, fun):
    """j_imd_d of COMPUTE_JOBS_D's criteria (NSE_D, KGE_D, SE_D, RMSE_D, LOGARITHMIC_D) and the value they return beside it"""
    n, two, one, z = T(S["n"]), T(2), T(1), T(0)
    if fun == "nse":
        mean_x = S["sx"] / n
        den = S["sxx"] - n * mean_x * mean_x
        return (S["syy_d"] - two * S["sxy_d"]) / den, (S["sxx"] - two * S["sxy"] + S["syy"]) / den
    if fun in ("kge", "kge2"):
        mean_x, mean_y_d, mean_y = S["sx"] / n, S["sy_d"] / n, S["sy"] / n
        var_x = S["sxx"] / n - mean_x * mean_x
        var_y_d, var_y = S["syy_d"] / n - two * mean_y * mean_y_d, S["syy"] / n - mean_y * mean_y
        cov_d, cov = S["sxy_d"] / n - mean_x * mean_y_d, S["sxy"] / n - mean_x * mean_y
        sx, sy = np.sqrt(var_x), np.sqrt(var_y)
        sy_d = z if var_y == 0 else var_y_d / (two * sy)
        r = cov / (sx * sy)
        r_d = (cov_d - r * sx * sy_d) / (sx * sy)
        a_d, a = sy_d / sx, sy / sx
        b_d, b = mean_y_d / mean_x, mean_y / mean_x
        arg1_d = two * (r - one) * r_d + two * (b - one) * b_d + two * (a - one) * a_d
        arg1 = (r - one) * (r - one) + (b - one) * (b - one) + (a - one) * (a - one)
        kv = np.sqrt(arg1)
        kd = z if arg1 == 0 else arg1_d / (two * kv)
        return (kd, kv) if fun == "kge" else (two * kv * kd, kv * kv)
    if fun == "se":
        return S["se_d"], S["se"]
    if fun == "rmse":
        tv = np.sqrt(S["se"] / n)
        return (z if S["se"] / n == 0 else S["se_d"] / (two * tv * n)), tv
    return S["lg_d"], S["lg"]


def _adjoint(T, S, fun, x, y, res_b, y_b):
    """y_b += the criterion's adjoint for the seed res_b (NSE_B, KGE_B, SE_B, RMSE_B, LOGARITHMIC_B), last step first"""
    n, two, z = T(S["n"]), T(2), T(0)
    counted = [i for i in range(x.size - 1, -1, -1) if x[i] >= 0]
    if fun == "nse":
        mean_x = S["sx"] / n
        num_b = res_b / (S["sxx"] - n * mean_x * mean_x)
        c_yy, c_xy = num_b, -(two * num_b)
        for i in counted:
            y_b[i] = y_b[i] + x[i] * c_xy + two * y[i] * c_yy
    elif fun in ("kge", "kge2"):
        k = _kge(T, S)
        if fun == "kge2":
            res_b = two * np.sqrt(k["arg1"]) * res_b
        arg1_b = z if k["arg1"] == 0 else res_b / (two * np.sqrt(k["arg1"]))
        one = T(1)
        r_b, b_b, a_b = two * (k["r"] - one) * arg1_b, two * (k["b"] - one) * arg1_b, two * (k["a"] - one) * arg1_b
        result1, result2 = np.sqrt(k["var_x"]), np.sqrt(k["var_y"])
        result1_b = a_b / np.sqrt(k["var_x"])
        var_y_b = z if k["var_y"] == 0 else result1_b / (two * np.sqrt(k["var_y"]))
        temp_b = r_b / (result1 * result2)
        cov_b = temp_b
        result2_b = -(k["cov"] * temp_b / result2)
        if not k["var_y"] == 0:
            var_y_b = var_y_b + result2_b / (two * np.sqrt(k["var_y"]))
        mean_y_b = b_b / k["mean_x"] - k["mean_x"] * cov_b - two * k["mean_y"] * var_y_b
        c_xy, c_yy, c_y = cov_b / n, var_y_b / n, mean_y_b / n
        for i in counted:
            y_b[i] = y_b[i] + x[i] * c_xy + two * y[i] * c_yy + c_y
    elif fun in ("se", "rmse"):
        if fun == "rmse":
            res_b = z if S["se"] / n == 0 else res_b / (n * two * np.sqrt(S["se"] / n))
        for i in counted:
            y_b[i] = y_b[i] - two * (x[i] - y[i]) * res_b
    else:
        for i in range(x.size - 1, -1, -1):
            if x[i] > 0 and y[i] > 0:
                arg1 = arg2 = y[i] / x[i]
                arg1_b = _log(T, arg2) * x[i] * res_b / arg1
                arg2_b = _log(T, arg1) * x[i] * res_b / arg2
                y_b[i] = y_b[i] + arg2_b / x[i] + arg1_b / x[i]


def heap_sort_idx(arr, idx):
    """heap_sort (mwd_cost.f90:594-673) on the list arr with the permutation idx carried along"""
    n = len(arr)
    if n < 2:
        return
    l, ir = n // 2 + 1, n
    while True:
        if l > 1:
            l -= 1
            a, ia = arr[l - 1], idx[l - 1]
        else:
            a, ia = arr[ir - 1], idx[ir - 1]
            arr[ir - 1], idx[ir - 1] = arr[0], idx[0]
            ir -= 1
            if ir == 1:
                arr[0], idx[0] = a, ia
                return
        i, j = l, l + l
        while j <= ir:
            if j < ir and arr[j - 1] < arr[j]:
                j += 1
            if a < arr[j - 1]:
                arr[i - 1], idx[i - 1] = arr[j - 1], idx[j - 1]
                i = j
                j = j + j
            else:
                j = ir + 1
        arr[i - 1], idx[i - 1] = a, ia


def tie_report(c, r):
    """of a median case c and its restatement r: (the gauges with equal gauge_jobs, the gauges at the two interpolation points, the
    gauges that receive a seed, the gauges a STABLE sort would have handed it to)"""
    gj, k = r["gauge_jobs"], r["k"]
    neg = [g for g in range(c["ng"]) if c["wgauge"][g] < 0]
    tied = [g for g in neg if sum(gj[h] == gj[g] for h in neg) > 1]
    order = sorted(neg, key=lambda g: (gj[g], g))
    stable = order[k - 1:k] if len(neg) % 2 else order[k - 1:k + 1]          # an odd count: the weight of the upper point is 0
    return tied, list(r["perm"][k - 1:k + 1]), tuple(sorted(r["seeded"])), tuple(sorted(stable))


def effective_wgauge(c):
    """the rule for a gauge without data: no qo >= 0 from the start step on counts as wgauge = 0"""
    qo = normalised(c)[0][:, c["start"] - 1:]
    return np.where((qo >= 0).any(axis=1), c["wgauge"], F32(0)).astype(F32)


def restate(c, dtype=F32, jobs_b=1.0, effective=True):
    """compute_jobs, COMPUTE_JOBS_B (seed jobs_b) and COMPUTE_JOBS_D of case c in dtype, sequential like the reference.  Returns a
    dict: jobs, qsim_b (ng, nt), jobs_d, and what the recipe checks the cases' claims on: n and gauge_jobs per gauge, the median's
    branch ("low", "high", "interp" or None), its index k, its sorted permutation and the gauges that receive its seed."""
    T = dtype
    ng, nt, s0 = c["ng"], c["nt"], c["start"] - 1
    w = (effective_wgauge(c) if effective else c["wgauge"]).astype(T)
    wj = c["wjobs"].astype(T)
    qo, qs, qd = normalised(c, T)
    z = T(0)
    out = dict(n=np.zeros(ng, int), gauge_jobs=np.full(ng, np.nan), branch=None, k=None, perm=None, seeded=())
    with np.errstate(all="ignore"):
        S, gj, gjd, gjt = [None] * ng, [z] * ng, [z] * ng, [z] * ng
        jobs, jobs_d, arr, arr_d, arr_t, arr_g = z, z, [], [], [], []
        for g in range(ng):
            if not (w[g] > 0 or w[g] < 0):
                continue
            S[g] = _sums(T, qo[g, s0:], qs[g, s0:], qd[g, s0:])
            out["n"][g] = S[g]["n"]
            j_imd = j_imd_d = j_imd_t = z
            for j, fun in enumerate(c["jobs"]):
                if S[g]["n"] > 0:
                    j_imd = _value(T, S[g], fun)
                    j_imd_d, j_imd_t = _tangent(T, S[g], fun)
                gj[g] = gj[g] + wj[j] * j_imd
                gjd[g] = gjd[g] + wj[j] * j_imd_d
                gjt[g] = gjt[g] + wj[j] * j_imd_t            # COMPUTE_JOBS_D sorts the values its own criteria return
            out["gauge_jobs"][g] = gj[g]
            if w[g] > 0:
                jobs = jobs + w[g] * gj[g]
                jobs_d = jobs_d + w[g] * gjd[g]
            else:
                arr.append(gj[g]); arr_d.append(gjd[g]); arr_t.append(gjt[g]); arr_g.append(g)
        jb = T(jobs_b)
        arr_b = [z] * len(arr)
        if arr:
            m = len(arr)
            srt, perm, srt_t, pt = list(arr), list(range(m)), list(arr_t), list(range(m))
            jobs, jobs_d = arr[0], arr_d[0]
            if m > 1:
                heap_sort_idx(srt, perm)
                heap_sort_idx(srt_t, pt)
                frac = T(m - 1) * T(0.5) + T(1)
                if frac <= 1:
                    out["branch"], jobs, jobs_d = "low", srt[0], arr_d[pt[0]]
                    arr_b[perm[0]] = arr_b[perm[0]] + jb
                elif frac >= m:
                    out["branch"], jobs, jobs_d = "high", srt[m - 1], arr_d[pt[m - 1]]
                    arr_b[perm[m - 1]] = arr_b[perm[m - 1]] + jb
                else:
                    k = int(frac)
                    f = frac - T(k)
                    out["branch"], out["k"] = "interp", k
                    jobs = srt[k - 1] + (srt[k] - srt[k - 1]) * f
                    jobs_d = arr_d[pt[k - 1]] + f * (arr_d[pt[k]] - arr_d[pt[k - 1]])
                    temp_b = f * jb
                    arr_b[perm[k]] = arr_b[perm[k]] + temp_b
                    arr_b[perm[k - 1]] = arr_b[perm[k - 1]] + (jb - temp_b)
            else:
                arr_b[0] = arr_b[0] + jb
            out["perm"] = [arr_g[i] for i in perm]
            out["seeded"] = tuple(arr_g[i] for i in range(m) if arr_b[i] != 0)
            jb = z
        qsim_b = np.zeros((ng, nt), T)
        for g in range(ng - 1, -1, -1):
            if not (w[g] > 0 or w[g] < 0):
                continue
            gauge_jobs_b = w[g] * jb if w[g] > 0 else arr_b[arr_g.index(g)]
            y_b = np.zeros(nt - s0, T)
            j_imd_b = z
            for j in range(len(c["jobs"]) - 1, -1, -1):
                j_imd_b = j_imd_b + wj[j] * gauge_jobs_b
                if S[g]["n"] > 0:
                    _adjoint(T, S[g], c["jobs"][j], qo[g, s0:], qs[g, s0:], j_imd_b, y_b)
                    j_imd_b = z
            qsim_b[g, s0:] = z + T(DT) * T(1e3) * y_b / T(c["area"][g])
    out.update(jobs=T(jobs), qsim_b=np.asfortranarray(qsim_b), jobs_d=T(jobs_d))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
W2 = (0.6, 0.4)
ALL6, W6 = CRIT, (0.3, 0.1, 0.15, 0.2, 0.15, 0.1)
NOLOG, W3 = ("nse", "kge", "rmse"), (0.5, 0.3, 0.2)     # the gauge cases: no libm call, bit for bit in both builds
_cases = None


def _gaps(kind):
    def edit(c, rng):
        s0, nt = c["start"] - 1, c["nt"]
        q = c["qobs"]
        if kind == "first":
            q[:, s0] = MISSING
        elif kind == "last":
            q[:, nt - 1] = MISSING
        elif kind == "block64":
            q[:, s0 + 64:s0 + 128] = MISSING                  # the second load of sx_k_cost_sums, whole
        elif kind == "n1":
            keep = q[:, s0 + 70].copy()
            q[:, s0:] = MISSING
            q[:, s0 + 70] = keep
        elif kind == "alternating":
            q[0, s0::2] = MISSING
            q[1, s0 + 1::2] = MISSING
    return edit


def _zero_obs(c, rng):
    s0 = c["start"] - 1
    c["qobs"][:, [s0, s0 + 7, s0 + 64]] = F32(0.0)
    c["qobs"][:, [s0 + 3, s0 + 63]] = F32(-0.0)               # counts for the sums (-0.0 >= 0), not for logarithmic
    c["qobs"][:, 1] = F32(-0.0)


def _zero_sim(c, rng):
    s0 = c["start"] - 1
    c["qsim"][:, [s0, s0 + 9, s0 + 64]] = F32(0.0)
    c["qsim"][:, [s0 + 4, s0 + 30]] = (F32(-0.01) * c["qsim"][:, [s0 + 4, s0 + 30]]).astype(F32)


def _equal(c, rng):
    c["qsim"] = c["qobs"].copy()                              # matched gauges: qs == qo bit for bit
    c["qobs"][:, c["start"] - 1 + 5] = MISSING                # ... on every COUNTED step; here they differ and are not counted


def _const_obs(c, rng):
    for g in range(c["ng"]):
        for t in range(c["start"] - 1, c["nt"]):
            _set_qo(c, g, t, 2.0)                             # sums of 2 and 4 are exact: den = 0 and var_x = 0 exactly


def _const_sim(c, rng):
    for g in range(c["ng"]):
        for t in range(c["start"] - 1, c["nt"]):
            _set_qs(c, g, t, 0.5)                             # var_y = 0 exactly


def _span(c, rng):
    s0, n = c["start"] - 1, c["nt"] - (c["start"] - 1)
    scale = (10.0 ** np.linspace(-6.0, 3.0, n))[rng.permutation(n)]
    c["qobs"][:, s0:] = (c["qobs"][:, s0:] * scale).astype(F32)
    c["qsim"][:, s0:] = (c["qsim"][:, s0:] * scale).astype(F32)
    c["qsim_d"][:, s0:] = (c["qsim_d"][:, s0:] * scale).astype(F32)


def cases():
    """{name: case} of the recorded cases, in a fixed order"""
    global _cases
    if _cases is not None:
        return _cases
    out = {}

    def add(name, *a, **kw):
        assert name not in out
        out[name] = _case(name, *a, seed=len(out), **kw)

    # -- the window: L = nt - s0 counted steps; s0 = 0, 5, 63, 64 and nt - 1
    for L, nt, s0 in ((1, 6, 5), (2, 2, 0), (63, 63, 0), (64, 69, 5), (65, 128, 63), (127, 191, 64), (128, 128, 0), (129, 134, 5), (200, 264, 64)):
        add(f"len{L}", 2, nt, s0, ALL6, W6, W2, claims=dict(n=[L, L]))
    # -- missing data, L = 129 behind five steps of junk
    for kind, n in (("first", 128), ("last", 128), ("block64", 65), ("n1", 1), ("alternating", None)):
        add(f"gaps_{kind}", 2, 134, 5, ALL6, W6, W2, edit=_gaps(kind), claims=dict(n=[n, n] if n else [64, 65]))
    # -- each criterion alone: on a plain series, and where it degenerates
    for j in CRIT:
        add(f"alone_{j}", 2, 134, 5, (j,), (1.0,), W2, claims=dict(n=[129, 129]))
        add(f"n1_{j}", 2, 134, 5, (j,), (1.0,), W2, edit=_gaps("n1"), claims=dict(n=[1, 1]))
        add(f"equal_{j}", 2, 70, 5, (j,), (1.0,), W2, matched=(0, 1), edit=_equal, claims=dict(n=[64, 64], equal=True))
    for j in ("nse", "kge", "kge2"):
        add(f"const_obs_{j}", 2, 70, 5, (j,), (1.0,), W2, edit=_const_obs, claims=dict(n=[65, 65], var_x0=True))
    for j in ("kge", "kge2"):
        add(f"const_sim_{j}", 2, 70, 5, (j,), (1.0,), W2, edit=_const_sim, claims=dict(n=[65, 65], var_y0=True))
    # -- values, all six criteria
    add("zero_obs", 2, 70, 5, ALL6, W6, W2, edit=_zero_obs, claims=dict(n=[65, 65]))
    add("zero_sim", 2, 70, 5, ALL6, W6, W2, edit=_zero_sim, claims=dict(n=[65, 65]))
    add("equal_all", 2, 70, 5, ALL6, W6, W2, matched=(0, 1), edit=_equal, claims=dict(n=[64, 64], equal=True))
    add("const_obs_all", 2, 70, 5, ALL6, W6, W2, edit=_const_obs, claims=dict(n=[65, 65], var_x0=True))
    add("const_sim_all", 2, 70, 5, ALL6, W6, W2, edit=_const_sim, claims=dict(n=[65, 65], var_y0=True))
    add("span", 2, 134, 5, ALL6, W6, W2, edit=_span, claims=dict(n=[129, 129]))
    add("span_nolog", 2, 134, 5, ("nse", "kge", "kge2", "se", "rmse"), (0.3, 0.1, 0.2, 0.2, 0.2), W2, edit=_span, claims=dict(n=[129, 129]))
    # -- njf = SX_MAXJF with repeats and one weight 0
    add("njf8", 3, 70, 5, ("nse", "kge", "nse", "se", "rmse", "logarithmic", "kge2", "kge"), (0.2, 0.1, 0.15, 0.0, 0.2, 0.1, 0.15, 0.1),
        (0.5, 0.3, 0.2), claims=dict(n=[65] * 3))
    add("njf8_nolog", 3, 70, 5, ("nse", "kge", "nse", "se", "rmse", "se", "kge2", "kge"), (0.2, 0.1, 0.15, 0.0, 0.2, 0.1, 0.15, 0.1),
        (0.5, 0.3, 0.2), claims=dict(n=[65] * 3))
    # -- gauges: nine steps, start step 3
    for ng in (1, 2, 3, 5, 64, 65, 70):
        w = 1.0 + np.arange(ng) % 7
        add(f"g{ng}", ng, 9, 2, NOLOG, W3, w / w.sum(), claims=dict(n=[7] * ng))
    for where, w in (("first", (0, .4, .3, .2, .1)), ("middle", (.4, .3, 0, .2, .1)), ("last", (.4, .3, .2, .1, 0))):
        add(f"zero_weight_{where}", 5, 9, 2, NOLOG, W3, w, claims=dict(n=[0 if v == 0 else 7 for v in w]))
    # -- the median: 1 .. 5 and 65 gauges with distinct values; ties at and off the interpolation points; mixed signs
    for m in (1, 2, 3, 4, 5):
        add(f"median{m}", m, 9, 2, NOLOG, W3, [-1.0] * m, claims=dict(n=[7] * m, median=m))
    w70 = -np.ones(70)
    w70[[0, 13, 40, 64, 69]] = (.3, .2, .2, .2, .1)
    add("median65_of_70", 70, 9, 2, NOLOG, W3, w70, claims=dict(n=[7] * 70, median=65))
    add("median_mixed", 5, 9, 2, NOLOG, W3, (.5, -1, .5, -1, -1), claims=dict(n=[7] * 5, median=3))
    # (where the twins' common value falls among the others is the draw's: the first seed that puts it where the name says, and
    # for "at" where the heap sort seeds other gauges than a stable sort would)
    for name, m, twins, tie in (("median_tie4_at", 4, (1, 2), "at"), ("median_tie5_at", 5, (0, 3), "at"), ("median_tie6_three", 6, (0, 2, 5), "at"),
                                ("median_tie5_off", 5, (1, 4), "off")):
        for seed in range(500, 700):
            c = _case(name, m, 9, 2, NOLOG, W3, [-1.0] * m, seed=seed, twins=twins, claims=dict(n=[7] * m, median=m, tie=tie))
            tied, pts, seeded, stable = tie_report(c, restate(c))
            if bool(set(pts) & set(tied)) == (tie == "at") and (tie == "off" or seeded != stable):
                break
        else:
            raise AssertionError(name)
        out[name] = c
    _cases = out
    return out


def _blank(*gauges, keep_before=False):
    def edit(c, rng):
        s0 = c["start"] - 1
        for g in gauges:
            c["qobs"][g, s0:] = MISSING
            if keep_before:
                c["qobs"][g, :s0] = MISSING
                c["qobs"][g, s0 - 1] = c["qobs"][(g + 1) % c["ng"], s0]       # its only observation: one step BEFORE the start step
    return edit


_empty = None


def empty_cases():
    """{name: (case, empty gauges)}: gauges with a non-zero weight and no observation from the start step on.  No reference: every
    output must equal the run with the weight of those gauges set to 0."""
    global _empty
    if _empty is None:
        _empty = {}
        pos, neg, mix = (.4, .3, .2, .1), (-1., -1., -1., -1.), (.5, -1., -1., -1.)
        for name, w, gs, kw in (("first", pos, (0,), {}), ("middle", pos, (2,), {}), ("last", pos, (3,), {}),
                                ("median_first", neg, (0,), {}), ("median_middle", neg, (1,), {}), ("median_last", neg, (3,), {}),
                                ("mixed_negative_empty", mix, (2,), {}), ("mixed_positive_empty", mix, (0,), {}),
                                ("two", pos, (1, 3), {}), ("all", pos, (0, 1, 2, 3), {}), ("all_median", neg, (0, 1, 2, 3), {}),
                                ("only_before_start", pos, (1,), dict(keep_before=True)),
                                ("only_before_start_median", neg, (2,), dict(keep_before=True))):
            _empty["empty_" + name] = (_case("empty_" + name, 4, 70, 5, ALL6, W6, w, seed=1000 + len(_empty), edit=_blank(*gs, **kw)), gs)
    return _empty


def with_weights(c, wgauge):
    return dict(c, wgauge=np.array(wgauge, F32))


def zeroed(c, gauges):
    w = c["wgauge"].copy()
    w[list(gauges)] = 0
    return with_weights(c, w)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
INPUTS = ("qobs", "qsim", "qsim_d", "wgauge", "wjobs", "gauge_pos", "flwacc", "area")


def load_fixture():
    """{name: dict(inputs as recorded, jobs, jobs_d, qsim_b1, qsim_b2, finite {criterion: bool})}"""
    z = np.load(FIXTURE)
    out = {}
    for name in [str(n) for n in z["cases"]]:
        r = {k: z[f"{name}__{k}"] for k in INPUTS + ("jobs", "jobs_d", "qsim_b1", "qsim_b2", "finite")}
        r["jobs_fun"] = tuple(str(j) for j in z[f"{name}__jobs_fun"])
        r["start"] = int(z[f"{name}__start"])
        r["finite"] = dict(zip(sorted(set(r["jobs_fun"]), key=CRIT.index), (bool(b) for b in r["finite"])))
        out[name] = r
    return out


# ---- gauges without data in a whole sweep ----------------------------------------------------------------------------------------------------
# On the small gr-b case full_5x13 of jreg_cases (two gauges, 12 steps, four regularisers): name -> the gauge weights, the gauges whose
# observations are blanked from the start step on, the start step, and whether such a gauge keeps one observation on the step BEFORE
# the start step.  "second" with (0.5, 0.5) is the case the rule was decided on: before it the forward and tangent sweeps dropped the
# gauge while the adjoint carried its seed into gauge 1 -- cost_d 1.01554 against <gradient, direction> 2.03109.
SWEEP_BASE = "full_5x13"
SWEEP_JOBS = dict(jobs_fun=("nse", "kge", "logarithmic"), wjobs_fun=(0.5, 0.3, 0.2))
SWEEP_EMPTY = {
    "second": dict(w=(0.5, 0.5), empty=(1,)),
    "first": dict(w=(0.5, 0.5), empty=(0,)),
    "median": dict(w=(-1.0, -1.0), empty=(1,)),
    "mixed": dict(w=(0.5, -1.0), empty=(1,)),
    "both": dict(w=(0.5, 0.5), empty=(0, 1)),
    "before_start": dict(w=(0.5, 0.5), empty=(1,), start=4, before=True),
}
_sweep_qobs = None


def sweep_case(name, zero=False, jobs=None):
    """case `name` of SWEEP_EMPTY as the namespace jreg_cases.build returns; zero: the empty gauges' weights set to 0 instead"""
    import jreg_cases as jc
    global _sweep_qobs
    if _sweep_qobs is None:
        _sweep_qobs = jc.build(SWEEP_BASE).qobs.copy()
    spec = SWEEP_EMPTY[name]
    start = spec.get("start", 1)
    q = _sweep_qobs.copy()
    for g in spec["empty"]:
        q[g, start - 1:] = MISSING
        if spec.get("before"):
            q[g, :start - 1] = MISSING
            q[g, start - 2] = _sweep_qobs[g, start - 2]
    w = np.array(spec["w"], F32)
    if zero:
        w[list(spec["empty"])] = 0
    g = jc.build(SWEEP_BASE, qobs=q)
    g.opts.update(jobs or SWEEP_JOBS, wgauge=w, optimize_start_step=start)
    g.id = f"empty_{name}" + ("_zero" if zero else "")
    return g


def shared_cell_case():
    """full_5x13 with BOTH gauges on the outlet cell, with areas, observations and weights of their own: sx_k_cost_cellseeds adds
    their seeds into the one cell in reverse gauge order (forward_db.f90:8650-8654).  smashx_jobs_of_qsim refuses shared cells, so
    this runs as a whole sweep."""
    import jreg_cases as jc
    from smash_amd import synth
    g = jc.build(SWEEP_BASE)
    m = g.mesh
    gp = [tuple(m.gauge_pos[0]), tuple(m.gauge_pos[0])]
    area = np.array([m.area[0], F32(0.8) * m.area[0]], F32)
    g.mesh = synth.Mesh(m.nrow, m.ncol, m.dx, m.flwdir, m.flwacc, m.path, m.active_cell, gp, area)
    q = g.qobs.copy()
    q[1] = (F32(1.1) * q[0]).astype(F32)
    q[1, 3] = MISSING
    g.qobs = np.asfortranarray(q)
    g.opts.update(SWEEP_JOBS, wgauge=np.array([0.6, 0.4], F32))
    g.id = "shared_cell"
    return g
