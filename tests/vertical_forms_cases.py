"""Inputs of tests/test_gpu_vertical_forms.py: a golden fixture's mesh, parameters and options with the forcing cut to nt steps and a
gap pattern applied.  Shared with tests/golden/vertical_forms/make_noise.py, which records the reference's own flag-to-flag noise on
every output of every case (tests/golden/vertical_forms/noise.npz) -- the cut inputs have no golden vector to take it from."""
import numpy as np

import golden_util as gu

BASE = "gr_b_16x16x96_nse_gaps"
# gr-a, gr-c: the fixtures of BASE's size; gr-d has none of that size, its smallest one stands in
OTHERS = ["gr_a_16x16x96_median3", "gr_c_16x16x96_kge_se_log_mask", "gr_d_12x12x48_rmse_kge2_start"]
NTS = [1, 2, 3, 7, 8, 9, 17]          # below, at and above one SX_HIK block, odd and even
# the other structures, one length: two blocks and a single step.  (It also leaves the cost criterion a window: the gr-d fixture starts
# its criterion at step 7, and over the three steps that 9 would leave, the reference's own two builds differ by 1e-4 .. 1e-3 on every
# gradient -- above golden_util.CAP, where a default-build bar is no parity bar.)
OTHER_NTS = [17]
PATTERNS = ["none", "own", "all_at_one_step", "one_cell_at_the_ends"]


def other_pattern(name, nt):
    """gr-a / gr-c / gr-d: the fixture's own gaps where it has some in the first nt steps, else one cell at the ends"""
    return "own" if (gu.load(name).prcp[:, :, :nt] < 0).any() else "one_cell_at_the_ends"


def all_cases():
    """(fixture, nt, pattern) of every case of the module"""
    out = [(BASE, nt, p) for nt in NTS + [33] for p in PATTERNS]
    out += [(BASE, 96, "own"), (BASE, 96, "one_cell_at_the_ends")]
    for name in OTHERS:
        for nt in OTHER_NTS:
            out += [(name, nt, other_pattern(name, nt)), (name, nt, "none")]
    return out


def _active_cell(g):
    """(row, col) of one active cell, well inside the list of active cells."""
    rows, cols = np.nonzero(np.asarray(g.mesh.active_cell) == 1)
    i = (2 * len(rows)) // 3
    return int(rows[i]), int(cols[i])


def make(name, nt, pattern):
    """The fixture cut to nt steps with the gap pattern applied; g.gap_steps: the steps the pattern put a gap at."""
    g = gu.load(name)
    assert nt <= g.nt
    g.nt = nt
    prcp, pet = np.array(g.prcp[:, :, :nt], order="F"), np.array(g.pet[:, :, :nt], order="F")
    if pattern != "own":
        prcp[prcp < 0] = 0.0                       # (the synthetic forcing has its gaps in the rain only)
        assert not (pet < 0).any()
    steps = []
    if pattern == "all_at_one_step":
        steps = [nt // 2]
        prcp[:, :, nt // 2] = -99.0
    elif pattern == "one_cell_at_the_ends":
        r, c = _active_cell(g)
        steps = sorted({t for t in (0, 1, nt - 2, nt - 1) if 0 <= t < nt})
        prcp[r, c, steps] = -99.0
    g.prcp, g.pet, g.qobs = prcp, pet, np.array(g.qobs[:, :nt], order="F")
    g.gap_steps = steps
    for a in (g.prcp, g.pet, g.qobs):
        a.setflags(write=False)
    return g


def outputs(structure, fwd, adj):
    """name -> array of every compared output, from a forward and an adjoint result dict (oracle.pyoracle.run / oracle.refbind.run)"""
    out = {"qsim": fwd["qsim"], "cost": np.float32(fwd["cost"]), "qsim (adjoint run)": adj["qsim"], "cost (adjoint run)": np.float32(adj["cost"])}
    out.update({"fstates." + k: fwd["fstates"][k] for k in gu.STRUCT_STATES[structure]})
    out.update({k + "_b": adj["parameters_b"][k] for k in gu.STRUCT_PARAMS[structure]})
    out.update({k + "_b": adj["states_b"][k] for k in gu.STRUCT_STATES[structure]})
    return out


def key(name, nt, pattern, output):
    return f"{name}|{nt}|{pattern}|{output}"
