"""One tangent direction per FIELD (or per cell) of a structure, and the CPU oracle's answers along it, for
tests/test_tangent_fields_cpu.py, tests/test_gpu_tangent_fields.py and the lone-field sweeps of tests/test_gpu_bounds.py.  A plain
helper module like bounds_cases.py.

Why per field.  Everything else in the suite runs the tangent model along a composite direction (1 % of every field at once).  On
the gr-b 16 x 16 x 96 fixture |qsim_d| is 10 along hft, 6 along hlr, 5.6 along lr, 2e-2 along ci or cp and 2e-3 along hi: a 1 % error
in the hi tangent moves the composite qsim_d by 1e-6 of its norm, which is the bar.  Along its own direction every field is the
whole answer.

Two anchors per field:
  * the truth rule of tests/test_gpu_parity_at_size.py, unchanged: rel_l2(hip, truth64) <= 2 rel_l2(oracle32, truth64) + 1e-6 per
    gauge, |hip - truth| <= 2 |ref - truth| + 3e-7 for cost_d (truth_failures);
  * the adjoint-tangent identity cost_d = <grad_f, d_f> against the gradient of the adjoint sweep of the same build:
    gap_hip <= 2 gap_ref32 + 2e-5 scale with scale = sum |g_i d_i| (identity_ok).  Tangent and adjoint take the same branches, so
    the identity stays well conditioned in fp32 where the truth rule does not.

Where it does not: the interception kink.  The fixtures' PET is exactly zero at night; sx_interception's min(pet, prcp + hi ci)
then sits on its kink with hi at a rounding distance of 0, and the SIGN of that rounding decides whether ei_d passes through.  fp32
and fp64 decide differently: along ci or hi alone the fp32 oracle is 5 .. 40 % away from the fp64 truth on gr-b and gr-c, and the
truth rule asserts nothing.  The "floor" variant of a case replaces every exactly zero PET value by 0.013 (gaps, < 0, and rain stay
as they are), which takes the trajectory off the kink: the fp32 oracle is then within 1e-4 of the truth along every field
(tests/test_tangent_fields_cpu.py), and the truth rule bites.  The "raw" variant keeps the fixture's forcing and takes the identity
only.

Every reference number is the plain-C oracle's (oracle/pyoracle.py: params_d, states_d, fp64, adjoint)."""
from __future__ import annotations

import numpy as np

import golden_util as gu
from smash_amd import synth

CASES = {"gr-a": "gr_a_12x12x48_nse", "gr-b": "gr_b_16x16x96_nse_gaps", "gr-c": "gr_c_16x16x96_kge_se_log_mask",
         "gr-d": "gr_d_12x12x48_rmse_kge2_start", "vic-a": "vic_a_16x16x96_nse_gaps"}
# A field whose direction runs on another fixture.  cp of gr-d on 12 x 12 x 48: cost_d is 2e-8, a difference of time sums that
# cancel to half of sum |g_i d_i|, and the fp32 oracle's own identity gap is 4.9e-4 of that scale in the floor variant -- above the
# 2e-4 within which a broken helper is told from rounding (tests/test_tangent_fields_cpu.py).  On 48 x 48 x 480 it is 1.2e-4 / 7.6e-5.
FIELD_CASE = {("gr-d", "cp"): "gr_d_48x48x480_nse"}
CELL_CASE = "gr_c_32x32x240_d8_ragged"
CELL_FIELDS = ("cft", "ci", "lr", "hft", "hlr")
VARIANTS = ("raw", "floor")
PET_FLOOR = np.float32(0.013)
# a field the structure does not read: its tangent is exactly zero in every build
UNUSED = {"gr-a": "ci", "gr-b": "cst", "gr-c": "b", "gr-d": "exc", "vic-a": "cp"}

E_REF_CAP = 1e-4                  # the fp32 oracle's distance from the truth above which the truth rule asserts nothing
IDENTITY_FACTOR = 2.0             # gap_hip <= IDENTITY_FACTOR gap_ref32 + IDENTITY_FLOOR scale
IDENTITY_FLOOR = 2e-5             # the bar of tests/test_gpu_tangent.py::test_scalar_product

DROW = (-1, -1, 0, 1, 1, 1, 0, -1)       # D8 codes 1..8 = N, NE, E, SE, S, SW, W, NW
DCOL = (0, 1, 1, 1, 0, -1, -1, -1)

_cases = {}
_adjoints = {}


def fields(structure):
    return gu.STRUCT_PARAMS[structure] + gu.STRUCT_STATES[structure]


def case_name(structure, f):
    return FIELD_CASE.get((structure, f), CASES[structure])


def floor_pet(pet):
    """A copy of pet with every exactly zero value at PET_FLOOR."""
    out = np.array(pet, np.float32, order="F", copy=True)
    out[out == 0] = PET_FLOOR
    return out


def load(name, variant="raw"):
    """Golden fixture name with the forcing of variant; loaded once, shared, not to be written to."""
    assert variant in VARIANTS, variant
    if (name, variant) not in _cases:
        g = gu.load(name)
        g.id = f"{name}:{variant}"
        if variant == "floor":
            g.pet = floor_pet(g.pet)
        g.direction = None
        _cases[name, variant] = g
    return _cases[name, variant]


def _zero_planes(g):
    z = lambda names: {k: np.zeros((g.mesh.nrow, g.mesh.ncol), np.float32, order="F") for k in names}
    return z(synth.PARAM_NAMES), z(synth.STATE_NAMES)


def _plane_of(g, f):
    return (g.params if f in synth.PARAM_NAMES else g.states)[f]


def field_direction(g, f):
    """(params_d, states_d): 0.01 max(|f|, 1e-3) on the active cells of field f, zero on every other cell and plane."""
    pd, sd = _zero_planes(g)
    d = np.float32(0.01) * np.maximum(np.abs(_plane_of(g, f)), np.float32(1e-3)).astype(np.float32)
    (pd if f in pd else sd)[f][...] = np.where(np.asarray(g.mesh.active_cell) == 1, d, np.float32(0))
    return pd, sd


def cell_direction(g, f, cell):
    """(params_d, states_d): 1 on cell (row, col) of field f, zero everywhere else."""
    pd, sd = _zero_planes(g)
    (pd if f in pd else sd)[f][cell] = np.float32(1)
    return pd, sd


def plane(direction, f):
    pd, sd = direction
    return pd[f] if f in pd else sd[f]


def _args(g):
    return g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states


def oracle_tangent(g, direction, fp64=False):
    """The oracle's tangent along direction: dict qsim_d (ng, nt), cost_d, qsim, as float64."""
    from oracle import pyoracle
    with np.errstate(all="ignore"):
        t = pyoracle.run(*_args(g), params_d=direction[0], states_d=direction[1], fp64=fp64, **g.opts)
    return {"qsim_d": np.asarray(t["qsim_d"], np.float64), "cost_d": float(t["cost_d"]), "qsim": np.asarray(t["qsim"], np.float64)}


def oracle_gradient(g, fp64=False):
    """The oracle's adjoint: dict field -> gradient plane, parameters and states of the structure.  Once per case and precision."""
    from oracle import pyoracle
    key = (getattr(g, "id", id(g)), fp64)
    if key not in _adjoints:
        with np.errstate(all="ignore"):
            b = pyoracle.run(*_args(g), adjoint=True, fp64=fp64, **g.opts)
        grad = {k: b["parameters_b"][k] for k in gu.STRUCT_PARAMS[g.structure]}
        grad.update({k: b["states_b"][k] for k in gu.STRUCT_STATES[g.structure]})
        _adjoints[key] = grad
    return _adjoints[key]


def _terms(grad, d):
    return np.asarray(grad, np.float64) * np.asarray(d, np.float64)


def gap(cost_d, grad, d):
    """|cost_d - sum g_i d_i|, the products and the sum in fp64."""
    return abs(float(cost_d) - float(np.sum(_terms(grad, d))))


def scale(grad, d):
    """sum |g_i d_i|"""
    return float(np.sum(np.abs(_terms(grad, d))))


def e_ref(ref32, ref64):
    """rel_l2(oracle32 qsim_d, truth64 qsim_d) per gauge."""
    return [gu.rel_l2(a, b) for a, b in zip(ref32["qsim_d"], ref64["qsim_d"])]


def identity_ok(gap_hip, gap_ref32, sc):
    return gap_hip <= IDENTITY_FACTOR * gap_ref32 + IDENTITY_FLOOR * sc


def truth_failures(label, hip, ref32, ref64):
    """The truth rule on qsim_d per gauge and on cost_d (hip: dict qsim_d, cost_d); one printed line per output, e_hip, e_ref and
    the distance from the fp32 oracle, as test_gpu_parity_at_size._check prints them.  Returns the names that fail."""
    bad = []
    for i in range(ref64["qsim_d"].shape[0]):
        h, r, t = np.asarray(hip["qsim_d"], np.float64)[i], ref32["qsim_d"][i], ref64["qsim_d"][i]
        e_hip, e_r = gu.rel_l2(h, t), gu.rel_l2(r, t)
        print(f"{label} qsim_d[{i}]  e_hip {e_hip:.2e}  e_ref {e_r:.2e}  vs oracle32 {gu.rel_l2(h, r):.2e}")
        if not e_hip <= 2.0 * e_r + 1e-6:
            bad.append(f"{label} qsim_d[{i}] e_hip {e_hip:.3e} e_ref {e_r:.3e}")
    h, r, t = float(hip["cost_d"]), ref32["cost_d"], ref64["cost_d"]
    e_hip, e_r = abs(h - t), abs(r - t)
    print(f"{label} cost_d     e_hip {e_hip:.2e}  e_ref {e_r:.2e}  vs oracle32 {abs(h - r):.2e}")
    if not e_hip <= 2.0 * e_r + 3e-7:
        bad.append(f"{label} cost_d e_hip {e_hip:.3e} e_ref {e_r:.3e}")
    return bad


def identity_failures(label, cost_d_hip, grad_hip, ref32, grad32, d):
    """The identity of one direction plane d on one field: the build's cost_d against its own gradient plane grad_hip, held to the
    fp32 oracle's own gap (ref32: oracle_tangent along the same direction, grad32: the oracle's gradient plane).  Prints both gaps
    relative to scale; returns the failures and (gap_hip / scale, gap_ref32 / scale)."""
    sc = scale(grad32, d)
    g_hip, g_ref = gap(cost_d_hip, grad_hip, d), gap(ref32["cost_d"], grad32, d)
    rel = (g_hip / sc, g_ref / sc) if sc > 0 else (g_hip, g_ref)
    print(f"{label} identity   gap_hip {g_hip:.2e} ({rel[0]:.2e} of scale)  gap_ref32 {g_ref:.2e} ({rel[1]:.2e})  scale {sc:.2e}")
    bad = [] if identity_ok(g_hip, g_ref, sc) else [f"{label} identity gap_hip {g_hip:.3e} gap_ref32 {g_ref:.3e} scale {sc:.3e}"]
    return bad, rel


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------
class Sweeps:
    """The adjoint sweep and any number of tangent sweeps of case g on ONE plan (the time of a small case is plan creation): the
    Solver that the first call makes stays on the case's input data and serves the later ones."""

    def __init__(self, g, **solver_kw):
        from test_gpu_parity import _types
        self.g = g
        self.setup, self.mesh, self.inp, _, _, _ = _types(g, **solver_kw)
        self._grad = None

    def _fields(self):
        import smash_amd
        return smash_amd.ParametersDT.from_dict(self.mesh, self.g.params), smash_amd.StatesDT.from_dict(self.mesh, self.g.states)

    def gradient(self):
        """field -> gradient plane of the adjoint sweep, parameters and states of the structure; swept once."""
        import smash_amd
        if self._grad is None:
            par, sta = self._fields()
            par_b, sta_b = par.copy(), sta.copy()
            o = smash_amd.OutputDT(self.setup, self.mesh)
            smash_amd.forward_b(self.setup, self.mesh, self.inp, par, par_b, self.inp._bgd[0], par.copy(), sta, sta_b, self.inp._bgd[1],
                                sta.copy(), o, o.copy(), np.float32(0), np.float32(1))
            self._grad = {k: getattr(par_b, k).copy() for k in gu.STRUCT_PARAMS[self.g.structure]}
            self._grad.update({k: getattr(sta_b, k).copy() for k in gu.STRUCT_STATES[self.g.structure]})
        return self._grad

    def tangent(self, direction):
        """dict qsim_d, cost_d, qsim of the tangent sweep along direction = (params_d, states_d)."""
        import smash_amd
        par, sta = self._fields()
        par_d = smash_amd.ParametersDT.from_dict(self.mesh, direction[0])
        sta_d = smash_amd.StatesDT.from_dict(self.mesh, direction[1])
        o, o_d = smash_amd.OutputDT(self.setup, self.mesh), smash_amd.OutputDT(self.setup, self.mesh)
        _, cost_d = smash_amd.forward_d(self.setup, self.mesh, self.inp, par, par_d, self.inp._bgd[0], par.copy(), sta, sta_d,
                                        self.inp._bgd[1], sta.copy(), o, o_d)
        return {"qsim_d": o_d.qsim.copy(), "cost_d": cost_d, "qsim": o.qsim.copy()}

    def chunk_steps(self):
        """the length of the plan's storage chunks in time steps"""
        return self.inp._smashx_solver.chunking()[0]


# ---- single cells ----------------------------------------------------------------------------------------------------------------
def active_cells(mesh):
    """The active cells (row, col) in column-major order."""
    a = np.asarray(mesh.active_cell)
    return [(int(r), int(c)) for c in range(mesh.ncol) for r in range(mesh.nrow) if a[r, c] == 1]


def drains_to_a_gauge(mesh, cell):
    """Walk the D8 plane down from cell: True if the path meets a gauge cell (the cell itself included)."""
    gauges = {(int(r), int(c)) for r, c in np.asarray(mesh.gauge_pos)}
    a, fd = np.asarray(mesh.active_cell), np.asarray(mesh.flwdir)
    r, c = cell
    for _ in range(mesh.nrow * mesh.ncol + 1):
        if not (0 <= r < mesh.nrow and 0 <= c < mesh.ncol) or a[r, c] != 1:
            return False
        if (r, c) in gauges:
            return True
        d = int(fd[r, c])
        if d < 1:
            return False
        r, c = r + DROW[d - 1], c + DCOL[d - 1]
    raise AssertionError("the flow directions loop")


def without_first_gauge(g):
    """A copy of case g without its first gauge.  In every golden fixture the first gauge is the outlet of the whole mesh, so that no
    cell lies outside every catchment; without it the cells below the other gauges drain to none."""
    import types
    m = g.mesh
    assert "wgauge" not in g.opts
    h = types.SimpleNamespace(**vars(g))
    h.id = getattr(g, "id", g.name) + ":no_outlet_gauge"
    h.mesh = synth.Mesh(m.nrow, m.ncol, m.dx, m.flwdir, m.flwacc, m.path, m.active_cell, np.asarray(m.gauge_pos)[1:].copy(),
                        np.asarray(m.area)[1:].copy())
    h.qobs = np.asfortranarray(g.qobs[1:])
    return h


def cell_sites(mesh):
    """name -> (row, col): the first and last active cell in column-major order, the cells at active positions 63 and 64 (a
    wavefront boundary of the vertical kernel) and the second gauge's cell (the first gauge of the mesh of without_first_gauge)."""
    cells = active_cells(mesh)
    assert len(cells) > 65
    gauge = tuple(int(v) for v in np.asarray(mesh.gauge_pos)[1])
    return {"first": cells[0], "last": cells[-1], "pos63": cells[63], "pos64": cells[64], "gauge": gauge}


def no_gauge_site(mesh):
    """One cell of mesh (a mesh of without_first_gauge) that drains to no gauge, found by walking the D8 plane down from every
    active cell: the one in the middle of the column-major list of such cells."""
    outside = [x for x in active_cells(mesh) if not drains_to_a_gauge(mesh, x)]
    assert outside, "every active cell drains to a gauge"
    return outside[len(outside) // 2]
