"""The reference's signature-based criteria restated in fp32 numpy, with their adjoint and tangent, and the loaders of the fixtures
tests/golden/make_signature_cost.py records from the compiled reference.

    signature, flow_percentile, quantile, heap_sort    smash/solver/optimize/mwd_cost.f90:594-970
    SIGNATURE_B / _D, FLOW_PERCENTILE_B / _D, QUANTILE_B / _D, HEAP_SORT_B / _D    smash/solver/forward/forward_db.f90:4030-4926

tests/test_signature_cost_cpu.py pins these functions bit for bit to the function-level fixtures; tests/test_gpu_signature_cost.py
holds the library to the same fixtures.  Every scalar is an np.float32 and every sum runs in time order, as in the reference."""
import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "signature_cost")
NAMES = ("Crc", "Cfp2", "Cfp10", "Cfp50", "Cfp90", "Epf", "Elt", "Erc")
CODES = {"nse": 1, "kge": 2, "kge2": 3, "se": 4, "rmse": 5, "logarithmic": 6,
         "Crc": 7, "Cfp2": 8, "Cfp10": 9, "Cfp50": 10, "Cfp90": 11, "Epf": 12, "Elt": 13, "Erc": 14}
PCT = {"Cfp2": np.float32(0.02), "Cfp10": np.float32(0.1), "Cfp50": np.float32(0.5), "Cfp90": np.float32(0.9)}
SET_ALL = ("nse", "Crc", "Cfp2", "Cfp10", "Cfp50", "Cfp90", "Epf", "Erc")
SET_MEDIAN = ("kge", "Elt", "Epf")
E2E_CASES = ("gr_a_cance_28x28x1440", "gr_b_16x16x96_nse_gaps")
F0, F1 = np.float32(0.0), np.float32(1.0)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def heap_sort_idx(arr):
    """heap_sort (mwd_cost.f90:594-673) with the permutation carried along: (sorted copy, idx) with sorted[k] = arr[idx[k]]"""
    a = f32(arr).copy()
    n = a.size
    idx = np.arange(n)
    if n < 2:
        return a, idx
    l, ir = n // 2 + 1, n
    while True:
        if l > 1:
            l -= 1
            al, il = a[l - 1], idx[l - 1]
        else:
            al, il = a[ir - 1], idx[ir - 1]
            a[ir - 1], idx[ir - 1] = a[0], idx[0]
            ir -= 1
            if ir == 1:
                a[0], idx[0] = al, il
                return a, idx
        i, j = l, l + l
        while j <= ir:
            if j < ir and a[j - 1] < a[j]:
                j += 1
            if al < a[j - 1]:
                a[i - 1], idx[i - 1] = a[j - 1], idx[j - 1]
                i, j = j, j + j
            else:
                j = ir + 1
        a[i - 1], idx[i - 1] = al, il


def quantile_points(dat, p):
    """quantile (mwd_cost.f90:675-723): (value, [(position in dat, weight rule)]) -- the one or two entries of dat the value reads, as
    (k1, k2, f): k2 = -1 and f = 0 when a single entry is read.  An empty dat reads the zeroed work array of flow_percentile."""
    dat = f32(dat)
    n = dat.size
    if n == 0:
        return F0, -1, -1, F0
    if n == 1:
        return dat[0], 0, -1, F0
    s, idx = heap_sort_idx(dat)
    frac = np.float32(np.float32(n - 1) * p) + F1
    if frac <= 1:
        return s[0], int(idx[0]), -1, F0
    if frac >= n:
        return s[n - 1], int(idx[n - 1]), -1, F0
    k = int(frac)
    f = np.float32(frac - np.float32(k))
    return np.float32(s[k - 1] + np.float32(np.float32(s[k] - s[k - 1]) * f)), int(idx[k - 1]), int(idx[k]), f


def flow_percentile(qo, qs, p):
    """flow_percentile (mwd_cost.f90:725-770): num, den, and the steps / weight behind num"""
    keep = np.flatnonzero((qo >= 0) & (qs >= 0))
    num, k1, k2, f = quantile_points(qs[keep], p)
    den = quantile_points(qo[keep], p)[0]
    return num, den, (int(keep[k1]) if k1 >= 0 else -1), (int(keep[k2]) if k2 >= 0 else -1), f


def events(mask):
    """n_event and (start, count) of every event as the reference finds them (mwd_cost.f90:805-831), 0-based starts"""
    mask = np.asarray(mask)
    pos = np.flatnonzero(mask > 0)
    nev = int(mask[pos[-1]]) if pos.size else 0
    out = []
    for i in range(1, nev + 1):
        w = np.flatnonzero(mask == i)
        out.append((int(w[0]) if w.size else 0, int(w.size)))
    return out


def _event_fold(po, qo, qs, a, cnt):
    s_qo = s_qs = s_po = m_qo = m_qs = m_po = F0
    i_qo = i_qs = i_po = 0
    for j in range(a, a + cnt):
        if qo[j] >= 0 and po[j] >= 0:
            s_qo = np.float32(s_qo + qo[j]); s_qs = np.float32(s_qs + qs[j]); s_po = np.float32(s_po + po[j])
            if qo[j] > m_qo:
                m_qo, i_qo = qo[j], j + 1
            if qs[j] > m_qs:
                m_qs, i_qs = qs[j], j + 1
            if po[j] > m_po:
                m_po, i_po = po[j], j + 1
    return s_qo, s_qs, s_po, m_qo, m_qs, m_po, i_qo, i_qs, i_po


class Unassigned(Exception):
    """the reference would read num / den before assigning them: the library refuses such inputs"""


def _walk(po, qo, qs, mask, name, qs_d=None):
    """signature (mwd_cost.f90:772-970) with SIGNATURE_B (res_b = 1) and, given qs_d, SIGNATURE_D: (res, qs_b, res_d)"""
    po, qo, qs = f32(po), f32(qo), f32(qs)
    n = qo.size
    qs_b = np.zeros(n, np.float32)
    qd = f32(qs_d) if qs_d is not None else np.zeros(n, np.float32)
    res = res_d = F0
    with np.errstate(all="ignore"):
        if name[0] == "E":
            ev = events(mask)
            nev = len(ev)
            num = den = None
            num_d = F0
            rec = []
            for (a, cnt) in ev:
                s_qo, s_qs, s_po, m_qo, m_qs, m_po, i_qo, i_qs, i_po = _event_fold(po, qo, qs, a, cnt)
                assigned = True
                if name == "Epf":
                    num, den = m_qs, m_qo
                    num_d = qd[i_qs - 1] if i_qs > 0 else F0
                elif name == "Elt":
                    num, den, num_d = np.float32(i_qs - i_po), np.float32(i_qo - i_po), F0
                elif s_po > 0:
                    num, den = np.float32(s_qs / s_po), np.float32(s_qo / s_po)
                    sd = F0
                    for j in range(a, a + cnt):
                        if qo[j] >= 0 and po[j] >= 0:
                            sd = np.float32(sd + qd[j])
                    num_d = np.float32(sd / s_po)
                else:
                    assigned = False
                    if den is None:
                        raise Unassigned(name)
                flag = 0
                if den > 0:
                    x = np.float32(np.float32(num / den) - F1)
                    if x >= 0:
                        res = np.float32(res + x); res_d = np.float32(res_d + np.float32(num_d / den)); flag = 1
                    else:
                        res = np.float32(res + (-x)); res_d = np.float32(res_d + (-np.float32(num_d / den))); flag = 2
                rec.append((a, cnt, s_po, i_qs, den, flag, assigned))
            rb = F1
            if nev > 0:
                res = np.float32(res / np.float32(nev)); res_d = np.float32(res_d / np.float32(nev)); rb = np.float32(rb / np.float32(nev))
            num_b = F0
            for (a, cnt, s_po, i_qs, den, flag, assigned) in reversed(rec):
                if flag == 1:
                    num_b = np.float32(num_b + np.float32(rb / den))
                elif flag == 2:
                    num_b = np.float32(num_b - np.float32(rb / den))
                if name == "Epf":
                    if i_qs > 0:
                        qs_b[i_qs - 1] = np.float32(qs_b[i_qs - 1] + num_b)
                    num_b = F0
                elif name == "Elt":
                    num_b = F0
                elif assigned:
                    c = np.float32(num_b / s_po)
                    num_b = F0
                    for j in range(a + cnt - 1, a - 1, -1):
                        if qo[j] >= 0 and po[j] >= 0:
                            qs_b[j] = np.float32(qs_b[j] + c)
            return res, qs_b, res_d
        k1 = k2 = -1
        f = F0
        if name == "Crc":
            m = (qo >= 0) & (po >= 0)
            s_qo = s_qs = s_po = sd = F0
            for j in np.flatnonzero(m):
                s_qo = np.float32(s_qo + qo[j]); s_qs = np.float32(s_qs + qs[j]); s_po = np.float32(s_po + po[j]); sd = np.float32(sd + qd[j])
            if not s_po > 0:
                raise Unassigned(name)
            num, den, num_d = np.float32(s_qs / s_po), np.float32(s_qo / s_po), np.float32(sd / s_po)
        else:
            num, den, k1, k2, f = flow_percentile(qo, qs, PCT[name])
            num_d = F0
            if k2 >= 0:
                num_d = np.float32(qd[k1] + np.float32(f * np.float32(qd[k2] - qd[k1])))
            elif k1 >= 0:
                num_d = qd[k1]
        num_b = F0
        if den > 0:
            x = np.float32(np.float32(num / den) - F1)
            if x >= 0:
                res, res_d, num_b = x, np.float32(num_d / den), np.float32(F1 / den)
            else:
                res, res_d, num_b = np.float32(-x), np.float32(-np.float32(num_d / den)), np.float32(-np.float32(F1 / den))
        if name == "Crc":
            qs_b[m] = np.float32(F0 + np.float32(num_b / s_po))
        else:
            tb = np.float32(f * num_b)          # (every seed is ADDED to a zero: a -0 weight leaves +0, forward_db.f90:4220, 4468)
            if k2 >= 0:
                qs_b[k2] = np.float32(F0 + tb)
            if k1 >= 0:
                qs_b[k1] = np.float32(F0 + np.float32(num_b - tb))
        return res, qs_b, res_d


def signature(po, qo, qs, mask, name):
    return _walk(po, qo, qs, mask, name)[0]


def signature_b(po, qo, qs, mask, name):
    """qs_b as SIGNATURE_B leaves it from zeros with res_b = 1"""
    return _walk(po, qo, qs, mask, name)[1]


def signature_d(po, qo, qs, qs_d, mask, name):
    return _walk(po, qo, qs, mask, name, qs_d)[2]


def refused(po, qo, mask, name):
    """True where the reference would read an unassigned num / den (independent of qs)"""
    try:
        _walk(po, qo, np.zeros_like(f32(qo)), mask, name)
        return False
    except Unassigned:
        return True


def stable_points(qo, qs, p):
    """the steps a STABLE sort would put at the interpolation points of flow_percentile (what the heap sort must be told from)"""
    keep = np.flatnonzero((qo >= 0) & (qs >= 0))
    n = keep.size
    if n < 2:
        return (int(keep[0]) if n else -1), -1
    order = np.argsort(qs[keep], kind="stable")
    frac = np.float32(np.float32(n - 1) * p) + F1
    if frac <= 1:
        return int(keep[order[0]]), -1
    if frac >= n:
        return int(keep[order[n - 1]]), -1
    k = int(frac)
    return int(keep[order[k - 1]]), int(keep[order[k]])


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def load_functions():
    """{case: dict(po, qo, qs, mask, qs_d, crit = {name: (res, qs_b, res_d)})} of tests/golden/signature_cost/functions.npz"""
    z = np.load(os.path.join(DIR, "functions.npz"))
    out = {}
    for case in [str(c) for c in z["cases"]]:
        d = {k: z[f"{case}__{k}"] for k in ("po", "qo", "qs", "mask", "qs_d")}
        d["crit"] = {nm: (z[f"{case}__{nm}__res"], z[f"{case}__{nm}__qs_b"], z[f"{case}__{nm}__res_d"])
                     for nm in NAMES if f"{case}__{nm}__res" in z.files}
        out[case] = d
    return out


def load_e2e(case, tag):
    return np.load(os.path.join(DIR, f"{case}__{tag}.npz"))


def same_bits(a, b):
    a, b = f32(a), f32(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
