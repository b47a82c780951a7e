"""fp32 numpy restatement of mw_interception_store::adjust_interception_store (smash/solver/routine/mw_interception_store.f90:19-160),
vectorised over cells and candidates -- arrays (cells, 49), a Python loop over time -- and the loader of the fixtures recorded from
the compiled reference (tests/golden/interception/*.npz, made by tests/golden/make_interception.py).

Every operation is a single IEEE fp32 operation in the reference's order (numpy float32 arithmetic neither contracts nor widens), the
result is a discrete choice, so the restatement equals the reference bit for bit: tests/test_interception_cpu.py pins it against the
fixtures, and it is the yardstick where the reference cannot go (tests/test_gpu_interception.py at size)."""
import os

import numpy as np

import golden_util as gu

DIR = os.path.join(gu.GOLDEN_DIR, "interception")
# fixture -> the golden case whose forcing and mesh it runs on (the forcing is not stored twice)
CASES = {
    "gr_b_16x16x96_nse_gaps": "gr_b_16x16x96_nse_gaps",
    "gr_b_16x16x96_nse_gaps__start17": "gr_b_16x16x96_nse_gaps",      # the run starts at 17:00: first and last day are partial
    "gr_c_32x32x240_d8_ragged": "gr_c_32x32x240_d8_ragged",
    "gr_a_cance_28x28x1440": "gr_a_cance_28x28x1440",                 # recorded as gr-b (gr-a has no interception store)
}

F = np.float32


def candidates():
    """cmax of the reference: ceiling((stp - stt) / step) entries stt + (i - 1) * step in fp32 (arange_r, m_array_creation.f90:41-54)"""
    stt, stp, step = F(0.1), F(5.0), F(0.1)
    n = int(np.ceil((stp - stt) / step))
    return stt + np.arange(n).astype(F) * step


def adjust(prcp, pet, day_index):
    """prcp, pet (cells, nt) float32, day_index (nt): the capacity of every cell, float32 (cells)."""
    prcp, pet = np.asarray(prcp, F), np.asarray(pet, F)
    nc, nt = prcp.shape
    day = np.asarray(day_index)
    assert day.shape == (nt,)
    # daily totals in time order, then min(daily prcp, daily pet) summed over the days in order
    daily = np.zeros(nc, F)
    dp, de = np.zeros(nc, F), np.zeros(nc, F)
    for t in range(nt):
        if t > 0 and day[t] != day[t - 1]:
            daily = daily + np.minimum(dp, de)
            dp, de = np.zeros(nc, F), np.zeros(nc, F)
        dp = dp + prcp[:, t]
        de = de + pet[:, t]
    daily = daily + np.minimum(dp, de)
    # every candidate from an empty store: gr_interception (md_gr_operator.f90:20-34), then sum += ec
    cmax = candidates()[None, :]
    h = np.zeros((nc, cmax.shape[1]), F)
    acc = np.zeros_like(h)
    one, zero = F(1.0), F(0.0)
    for t in range(nt):
        p, e = prcp[:, t][:, None], pet[:, t][:, None]
        ei = np.minimum(e, p + h * cmax)
        pn = np.maximum(zero, p - cmax * (one - h) - ei)
        h = h + (p - ei - pn) / cmax
        acc = acc + ei
    diff = np.abs(acc - daily[:, None])
    assert diff.dtype == F and h.dtype == F
    return cmax[0][np.argmin(diff, axis=1)], diff          # argmin: the first minimum, like minloc


def exact_ties(diff):
    """number of cells whose two smallest differences are exactly equal"""
    s = np.sort(diff, axis=1)
    return int(np.sum(s[:, 0] == s[:, 1]))


def load(name):
    """(golden case, day_index, nday, ci plane (nrow, ncol)) of a recorded fixture"""
    z = np.load(os.path.join(DIR, name + ".npz"))
    return gu.load(CASES[name]), z["day_index"], int(z["nday"]), np.asfortranarray(z["ci"])


def active_columns(g):
    """forcing of the active cells as (cells, nt) arrays plus their (rows, cols)"""
    rows, cols = np.nonzero(np.asarray(g.mesh.active_cell) == 1)
    return g.prcp[rows, cols, :], g.pet[rows, cols, :], rows, cols
