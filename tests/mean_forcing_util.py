"""fp32 numpy restatement of mw_forcing_statistic::compute_mean_forcing (smash/solver/routine/mw_forcing_statistic.f90:18-75) and the
loader of the fixtures recorded from the compiled reference (tests/golden/mean_forcing/*.npz, made by
tests/golden/make_mean_forcing.py).

Per gauge and step the reference forms sum(matrix, mask = matrix >= 0 and upstream(gauge)) / count(mask): a sequential fp32 sum over
the cells in column-major order (row index fastest), one conversion of the count and one division.  Here the masked values of all
steps are laid out (cells, nt) with zeros where the mask is false -- x + 0 = x for every x the sum can hold, it never holds -0 -- and
np.add.accumulate runs down the cell axis: sequential along that axis, vectorised over the steps.  tests/test_mean_forcing_cpu.py
pins the restatement to the fixtures bit for bit; it is the yardstick where the reference cannot go."""
import os

import numpy as np

import golden_util as gu

DIR = os.path.join(gu.GOLDEN_DIR, "mean_forcing")
# fixture -> the golden case whose forcing and mesh it runs on (the forcing is not stored twice)
CASES = {
    "gr_a_cance_28x28x1440": "gr_a_cance_28x28x1440",
    "gr_b_16x16x96_nse_gaps": "gr_b_16x16x96_nse_gaps",
    "gr_b_16x16x96_nse_gaps__blank": "gr_b_16x16x96_nse_gaps",
    "gr_c_32x32x240_d8_ragged": "gr_c_32x32x240_d8_ragged",
    "gr_b_64x64x720_nse": "gr_b_64x64x720_nse",
}
# the __blank variant: these steps are set to -99 on every cell, so that count = 0 and the mean is 0 / 0
BLANK = {"gr_b_16x16x96_nse_gaps__blank": dict(prcp=(7, 64), pet=(31,))}

F = np.float32
# D8 codes 1..8: the neighbour at (row + DROW[i], col + DCOL[i]) drains into (row, col) when its code is i + 1 (mw_mask.f90:29-31)
DROW = (1, 1, 0, -1, -1, -1, 0, 1)
DCOL = (0, -1, -1, -1, 0, 1, 1, 1)


def upstream(flwdir, row, col):
    """mask_upstream_cells (mw_mask.f90:11-54) without recursion: the (nrow, ncol) mask of (row, col), 0-based, and of every cell whose D8
    path reaches it, over the whole grid (active or not)"""
    flwdir = np.asarray(flwdir)
    nrow, ncol = flwdir.shape
    mask = np.zeros((nrow, ncol), bool)
    mask[row, col] = True
    stack = [(int(row), int(col))]
    while stack:
        r, c = stack.pop()
        for i in range(8):
            rn, cn = r + DROW[i], c + DCOL[i]
            if 0 <= rn < nrow and 0 <= cn < ncol and flwdir[rn, cn] == i + 1 and not mask[rn, cn]:
                mask[rn, cn] = True
                stack.append((rn, cn))
    return mask


def gauge_masks(mesh):
    gp = np.asarray(mesh.gauge_pos).reshape(-1, 2)
    return [upstream(mesh.flwdir, gp[g, 0], gp[g, 1]) for g in range(gp.shape[0])]


def _sequential(values, valid):
    """values, valid (cells, nt) in summation order: (sum, count) per step, the sum sequential in fp32"""
    if values.shape[0] == 0:
        return np.zeros(values.shape[1], F), np.zeros(values.shape[1], np.int64)
    x = np.where(valid, values, F(0)).astype(F)
    acc = np.add.accumulate(x, axis=0, dtype=F)
    return acc[-1], valid.sum(axis=0)


def mean_forcing(flwdir, gauge_pos, prcp, pet, counts=False):
    """prcp, pet (nrow, ncol, nt) float32; gauge_pos (ng, 2) 0-based -> mean_prcp, mean_pet (ng, nt) float32, Fortran order.
    counts = True: also the two (ng, nt) count arrays."""
    prcp, pet = np.asarray(prcp), np.asarray(pet)
    assert prcp.dtype == F and pet.dtype == F
    gp = np.asarray(gauge_pos).reshape(-1, 2)
    ng, nt = gp.shape[0], prcp.shape[2]
    out = [np.zeros((ng, nt), F, order="F") for _ in range(2)]
    cnt = [np.zeros((ng, nt), np.int64) for _ in range(2)]
    for g in range(ng):
        mask = upstream(flwdir, gp[g, 0], gp[g, 1])
        cols, rows = np.nonzero(mask.T)                    # column-major order: the column index slowest
        for i, field in enumerate((prcp, pet)):
            v = field[rows, cols, :]
            s, c = _sequential(v, v >= 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[i][g, :] = s / c.astype(F)
            cnt[i][g, :] = c
    assert out[0].dtype == F
    return (out[0], out[1], cnt[0], cnt[1]) if counts else (out[0], out[1])


def fp64_means(flwdir, gauge_pos, prcp, pet):
    """the same means with the sum taken in float64 and rounded once: what a reassociated sum would be close to"""
    gp = np.asarray(gauge_pos).reshape(-1, 2)
    out = [np.zeros((gp.shape[0], prcp.shape[2]), F, order="F") for _ in range(2)]
    for g in range(gp.shape[0]):
        mask = upstream(flwdir, gp[g, 0], gp[g, 1])
        for i, field in enumerate((prcp, pet)):
            v = field[mask].astype(np.float64)
            ok = v >= 0
            with np.errstate(invalid="ignore", divide="ignore"):
                out[i][g, :] = np.where(ok, v, 0.0).sum(axis=0).astype(F) / ok.sum(axis=0).astype(F)
    return out


def blanked(name, prcp, pet):
    """the forcing of a fixture: the golden case's, with the variant's steps set to -99 on every cell"""
    b = BLANK.get(name)
    if b is None:
        return prcp, pet
    prcp, pet = prcp.copy(order="F"), pet.copy(order="F")
    prcp[:, :, list(b["prcp"])] = F(-99.0)
    pet[:, :, list(b["pet"])] = F(-99.0)
    return prcp, pet


def load(name):
    """(golden case, prcp, pet, mean_prcp, mean_pet) of a recorded fixture; prcp / pet are the variant's forcing"""
    z = np.load(os.path.join(DIR, name + ".npz"))
    g = gu.load(CASES[name])
    prcp, pet = blanked(name, g.prcp, g.pet)
    return g, prcp, pet, np.asfortranarray(z["mean_prcp"]), np.asfortranarray(z["mean_pet"])


def same_bits(a, b):
    """fp32 bit patterns equal, NaN positions compared as NaN on both sides (the host's 0 / 0 carries a sign bit the device's does not)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def count_differing(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.sum((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))))
