"""fp32 numpy restatement of mw_forcing_statistic::compute_prcp_indices (smash/solver/routine/mw_forcing_statistic.f90:77-220) and the
loader of the fixtures recorded from the compiled reference (tests/golden/prcp_indices/*.npz, made by
tests/golden/make_prcp_indices.py).

Per gauge, once: d = flwdst - flwdst(gauge) over the whole grid, its quantiles 0, 0.1 .. 1 over the catchment (quantile1d_r,
m_statistic.f90:231-277) and the cumulated bin counts wf.  Per gauge and step: a count and six sequential fp32 sums over the
catchment's cells with rain >= 0 in column-major order, ten plain sums over the distance bins of the WHOLE grid, and the closing
arithmetic (std, d1, d2, vg), every operation rounded on its own.  A step whose rain sum is not > 0 leaves its four entries as the
caller passed them.  pwf(1) reads the cell (gauge_row, gauge_row): the reference indexes the column with the gauge's row
(mw_forcing_statistic.f90:181), and so does this file.

The sums are laid out (cells, nt) with zeros where the mask is false -- x + 0 = x for every x a sum that starts at +0 can hold -- and
np.add.accumulate runs down the cell axis: sequential along that axis, vectorised over the steps.  tests/test_prcp_indices_cpu.py
pins the restatement to the fixtures bit for bit; it is the yardstick where the reference cannot go."""
import os

import numpy as np

import golden_util as gu
from mean_forcing_util import count_differing, same_bits, upstream  # noqa: F401

DIR = os.path.join(gu.GOLDEN_DIR, "prcp_indices")
# fixture -> the golden case whose rain and mesh it runs on (the forcing is not stored twice)
CASES = {
    "gr_a_cance_28x28x1440": "gr_a_cance_28x28x1440",
    "gr_b_16x16x96_nse_gaps": "gr_b_16x16x96_nse_gaps",
    "gr_b_16x16x96_nse_gaps__wet": "gr_b_16x16x96_nse_gaps",
    "gr_c_32x32x240_d8_ragged": "gr_c_32x32x240_d8_ragged",
    "gr_b_64x64x720_nse": "gr_b_64x64x720_nse",
}
# The rain of gr_b_16x16x96_nse_gaps falls on 14 of its 96 steps: 40 (gauge, step) pairs are written, fewer than the 64 the recorder
# asks of a case.  The case is recorded as it is (FEW_WRITTEN: the one condition it is let off, every other one holds) and again as the
# __wet variant, which meets them all: every dry step takes the rain plane of a wet step, in turn, under its OWN gap pattern; one
# step in eight stays dry.
FEW_WRITTEN = {"gr_b_16x16x96_nse_gaps": 40}
WET = ("gr_b_16x16x96_nse_gaps__wet",)
SENTINEL = np.float32(-7.0)
F = np.float32
NQ = 11


def quantiles_wf(d1d):
    """d1d: the catchment's distances (any order, at least 2) -> (flwdst_qtl, wf), 11 float32 each"""
    b = np.sort(np.asarray(d1d, F))
    n = b.size
    assert n >= 2, "quantile1d_r reads b(2)"
    qtl = np.zeros(NQ, F)
    for i in range(NQ):
        q = F(10 * i) / F(100)
        if q >= F(1):
            qtl[i] = b[n - 1]
        else:
            div = F(q * F(n - 1)) + F(1)
            qt = int(np.floor(div))
            r = np.fmod(div, F(qt))
            qtl[i] = F(F(F(1) - r) * b[qt - 1]) + F(r * b[qt])
    wf = np.zeros(NQ, F)
    wf[0] = F(1)
    for j in range(1, NQ):
        wf[j] = wf[j - 1] + F(np.count_nonzero((b > qtl[j - 1]) & (b <= qtl[j])))
    return qtl, wf


def _seq32(x):
    """(cells, nt) float32 -> the sequential fp32 sum down the cells"""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1], F)
    return np.add.accumulate(x.astype(F, copy=False), axis=0, dtype=F)[-1]


def _wide(x):
    """the same sum taken in float64 and rounded once"""
    return x.astype(np.float64).sum(axis=0).astype(F)


def gauge_tables(flwdir, gauge_pos, flwdst):
    """per gauge: dict(rows, cols: the catchment in column-major order; d: its distances; dgrid; qtl; wf; bins: ten (rows, cols) of the
    whole grid in column-major order)"""
    flwdst = np.asarray(flwdst)
    assert flwdst.dtype == F
    out = []
    for r, c in np.asarray(gauge_pos).reshape(-1, 2):
        mask = upstream(flwdir, r, c)
        cols, rows = np.nonzero(mask.T)                    # column-major order: the column index slowest
        dgrid = (flwdst - flwdst[r, c]).astype(F)
        d = dgrid[rows, cols]
        qtl, wf = quantiles_wf(d)
        bins = []
        for k in range(1, NQ):
            bc, br = np.nonzero(((dgrid > qtl[k - 1]) & (dgrid <= qtl[k])).T)
            bins.append((br, bc))
        out.append(dict(row=int(r), col=int(c), rows=rows, cols=cols, d=d, dgrid=dgrid, qtl=qtl, wf=wf, bins=bins))
    return out


def prcp_indices(flwdir, gauge_pos, flwdst, prcp, out, wide=False, gauge_col=False):
    """out (4, ng, nt) float32 Fortran order, in place: (std, d1, d2, vg) on the steps with rain, untouched elsewhere.  Returns the
    (ng, nt) mask of the pairs written.  wide = True: every sum in float64 rounded once (what a reassociated sum is close to);
    gauge_col = True: pwf(1) from the cell (gauge_row, gauge_col) instead of the reference's (gauge_row, gauge_row)."""
    prcp = np.asarray(prcp)
    assert prcp.dtype == F and out.dtype == F and out.shape[0] == 4
    add = _wide if wide else _seq32
    nt = prcp.shape[2]
    tabs = gauge_tables(flwdir, gauge_pos, flwdst)
    written = np.zeros((len(tabs), nt), bool)
    with np.errstate(all="ignore"):
        for g, T in enumerate(tabs):
            m = prcp[T["rows"], T["cols"], :]                  # (cells, nt)
            ok = m >= 0
            d = T["d"][:, None]
            zero = F(0)
            minv_n = F(1) / ok.sum(axis=0).astype(F)
            sum_p = add(np.where(ok, m, zero))
            sum_p2 = add(np.where(ok, m * m, zero))
            sum_d = add(np.where(ok, d, zero))
            sum_d2 = add(np.where(ok, d * d, zero))
            sum_pd = add(np.where(ok, m * d, zero))
            sum_pd2 = add(np.where(ok, (m * d) * d, zero))
            mean_p = p0 = minv_n * sum_p
            p1, p2, g1, g2 = minv_n * sum_pd, minv_n * sum_pd2, minv_n * sum_d, minv_n * sum_d2
            pwf = np.zeros((NQ, nt), F)
            pcell = prcp[T["row"], T["col"] if gauge_col else T["row"], :]
            pwf[0] = np.maximum(zero, pcell / sum_p)
            for k in range(1, NQ):
                br, bc = T["bins"][k - 1]
                mean_subp = np.zeros(nt, F) if br.size == 0 else add(prcp[br, bc, :]) / F(br.size)
                pwf[k] = pwf[k - 1] + (mean_subp / mean_p) * T["wf"][k]
            d1 = p1 / (p0 * g1)
            d2 = (F(1) / (g2 - g1 * g1)) * ((p2 / p0) - (p1 / p0) * (p1 / p0))
            std = np.sqrt((minv_n * sum_p2) - (mean_p * mean_p))
            vg = maxval(np.abs(pwf / pwf[NQ - 1] - (T["wf"] / T["wf"][NQ - 1])[:, None]))
            w = sum_p > 0
            for i, v in enumerate((std, d1, d2, vg)):
                assert v.dtype == F
                out[i, g, w] = v[w]
            written[g] = w
    return written


def maxval(a):
    """maxval down the first axis as the compiled reference forms it: the running maximum starts at the first element and is replaced
    where the next one compares greater, so a NaN that is not first is passed over and a NaN that is first stays"""
    acc = a[0].copy()
    for k in range(1, a.shape[0]):
        acc = np.where(a[k] > acc, a[k], acc)
    return acc


def rain(name, prcp):
    """the rain of a fixture: the golden case's, or the __wet variant of it"""
    if name not in WET:
        return prcp
    total = np.where(prcp >= 0, prcp, F(0)).sum(axis=(0, 1))
    wet = np.flatnonzero(total > 0)
    out = prcp.copy(order="F")
    for i, t in enumerate(np.flatnonzero(total == 0)):
        if t % 8 == 5:
            continue
        out[:, :, t] = np.where(prcp[:, :, t] < 0, prcp[:, :, t], np.abs(prcp[:, :, wet[i % wet.size]]))
    return out


def load(name):
    """(golden case, rain, flwdst, prcp_indices) of a recorded fixture; the rain is the variant's"""
    z = np.load(os.path.join(DIR, name + ".npz"))
    assert str(z["case"]) == CASES[name]
    g = gu.load(CASES[name])
    return g, rain(name, g.prcp), np.asfortranarray(z["flwdst"]), np.asfortranarray(z["prcp_indices"])


def sentinels(ng, nt):
    return np.full((4, ng, nt), SENTINEL, F, order="F")
