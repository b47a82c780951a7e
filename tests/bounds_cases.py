"""Small synthetic problems with one field AT A BOUND of the calibration box (or states outside it), and their CPU-oracle outputs
and branch census, for tests/test_bounds_cpu.py and tests/test_gpu_bounds.py.  A plain helper module like size_cases.py.

Everything else in the suite takes its parameters and states from the middle of the feasible box (synth.make_parameters /
make_states); a calibration does not stay there: L-BFGS-B projects onto GLB_P / GUB_P / GLB_S / GUB_S of oracle/refbind.py and
leaves whole regions of a field on a bound.  Out there the operators run on the edges of their hand-written shortcuts: tanh
saturated by pn / 1e-6, the transfer powers at the 1e-6 floor, prd + l <= 0 under exc = -50, the gap branch with a non-positive
base, the percolation power of a store above 15, interception capacities of 1e-6 and 100, routing with lr = 1e-6 and 1000, the
clamps of the vic-a operators.

Every case is rebuilt from its id alone:
  B:<structure>:<field>:<lb|ub>   12 x 12 cells, 2 gauges, 72 hourly steps of synthetic forcing with 2 % data gaps, warm states;
                                  <field> (a parameter or state of the structure) set to its bound on every second column, every
                                  other field at its synthetic value.  ONE field per case: corners of several fields at once
                                  overflow the fp32 reference.
  O:<structure>                   gr-b, gr-c, gr-d on 16 x 16 cells with states outside the box: hp = 20, hft = 1.2, hi = 1.5, each
                                  on its own random half of the cells (np.random.default_rng(11)).  O:vic-a: both upper layers
                                  full (husl1 = husl2 = 1, one step past the box) on one random half -- the only way to the clamp
                                  wusl >= cusl - 1e-6 and to iflc + prcp >= iflm, which no single field at a bound reaches.
Observations are the oracle's discharge at parameters + 10 % (no field at a bound); the tangent direction is 0.01 x every
parameter of the structure, with a zero state direction.  tangent_extras adds, per case, the same direction without ci (gr-b, gr-c)
and the direction of the field on the bound alone (states included), with the oracle's answers along them."""
from __future__ import annotations

import types

import numpy as np

import golden_util as gu
from smash_amd import synth

DT = 3600.0
NT = 72
GAPS = 20000                      # ppm
STRUCTURES = ("gr-a", "gr-b", "gr-c", "gr-d", "vic-a")
OUTSIDE = ("gr-b", "gr-c", "gr-d", "vic-a")
OUTSIDE_STATES = (("hp", 20.0), ("hft", 1.2), ("hi", 1.5))       # gr: in the order their masks are drawn
OUTSIDE_VIC = (("husl1", 1.0), ("husl2", 1.0))                   # vic-a: on the same (first) mask

# An initial routing state of 1e4 (GUB_S) makes the cost 4e7 and tests nothing else: the upper end of hlr is 50.
HLR_UB = 50.0
# The four corners at which the reference's own statements overflow (NaN in the fp32 and in the fp64 oracle at the bound itself): the
# value is moved inward by factors of 10 until every output of both oracles is finite.  (field, end): value used instead of the bound.
MOVED_IN = {
    ("cft", "lb"): 1e-1,          # gr_transfer's (ht ct)^-4 overflows fp32 up to 1e-2: discharge and cost NaN (fp64 finite from 1e-3)
    ("cst", "lb"): 1e-2,          # the same statement on the slow store: fp32 NaN up to 1e-3
    ("cusl2", "lb"): 1e2,         # forward finite, but the adjoint and tangent of the upper layers are NaN in both precisions up to 1e1
    ("ks", "ub"): 1e1,            # the same outputs: NaN in both precisions from 1e3, in fp32 at 1e2
}

# The census counters (oracle.pyoracle.CENSUS, defined in oracle/smash_oracle.h) that a case named for a regime must reach in the
# fp32 oracle: (field, end) -> (counters, structures that must reach them).  From the operators, not from a run of the kernels: e.g.
# hft can only fall to the 1e-6 floor where the exchange l < 0 outweighs pr + perc, which gr-d (no exchange) never has, and a store
# that starts on the floor leaves it at once where the first step brings rain (gr-a: no interception store to take it).
_GR = ("gr-a", "gr-b", "gr-c", "gr-d")
EXPECTED = {
    ("cp", "lb"): (("tanh_sat",), _GR),                                  # pn / 1e-6, en / 1e-6
    ("cft", "lb"): (("hft_floor",), ("gr-a", "gr-b", "gr-c")),
    ("hft", "lb"): (("hft_floor",), ("gr-b", "gr-c")),
    ("hst", "lb"): (("hst_floor",), ("gr-c",)),
    ("exc", "lb"): (("qd_zero",), ("gr-a", "gr-b", "gr-c")),             # (and more often than at exc = +50: test_bounds_cpu.py)
    ("ci", "lb"): (("ei_store", "calm_not_still"), ("gr-b", "gr-c")),    # hi leaves [0, 1]: the still-step shortcut must stand back
    ("ci", "ub"): (("ei_store", "pn_interception"), ("gr-b", "gr-c")),
    ("hi", "lb"): (("ei_store",), ("gr-b", "gr-c")),
    ("hi", "ub"): (("pn_interception",), ("gr-b", "gr-c")),
    ("b", "lb"): (("vic_ifl_prcp",), ("vic-a",)),
    ("cusl1", "lb"): (("vic_usl1_full", "vic_bc_limited", "vic_evap_store"), ("vic-a",)),
    ("cusl1", "ub"): (("vic_bc_room",), ("vic-a",)),
    ("cusl2", "lb"): (("vic_wusl_low",), ("vic-a",)),
    ("clsl", "lb"): (("vic_qb_store", "vic_bc_room"), ("vic-a",)),
    ("ws", "lb"): (("vic_above_ws", "vic_usl2_full"), ("vic-a",)),
    ("husl1", "ub"): (("vic_usl1_full",), ("vic-a",)),
    ("husl2", "ub"): (("vic_bc_room", "vic_bc_limited"), ("vic-a",)),
    ("hlsl", "ub"): (("vic_above_ws",), ("vic-a",)),
}
EXPECTED_OUTSIDE = {"gr-b": ("hp_big", "perc_pow", "gap_pwx3_nonpos", "calm_not_still", "hft_floor"),
                    "gr-c": ("hp_big", "perc_pow", "gap_pwx3_nonpos", "calm_not_still", "hft_floor"),
                    "gr-d": ("hp_big", "perc_pow", "gap_pwx3_nonpos", "calm_not_still"),
                    "vic-a": ("vic_wusl_high", "vic_ifl_full", "vic_usl1_full", "vic_usl2_full")}


def fields(structure):
    return gu.STRUCT_PARAMS[structure] + gu.STRUCT_STATES[structure]


def ids(structure=None):
    """The ids of every case (of one structure)."""
    out = []
    for s in STRUCTURES if structure is None else (structure,):
        out += [f"B:{s}:{f}:{e}" for f in fields(s) for e in ("lb", "ub")]
        if s in OUTSIDE:
            out.append(f"O:{s}")
    return out


def bound_value(field, end):
    """The value a B: case puts on every second column of field."""
    from oracle.refbind import GLB_P, GLB_S, GUB_P, GUB_S
    if (field, end) in MOVED_IN:
        return np.float32(MOVED_IN[field, end])
    if field == "hlr" and end == "ub":
        return np.float32(HLR_UB)
    if field in synth.PARAM_NAMES:
        return (GLB_P if end == "lb" else GUB_P)[synth.PARAM_NAMES.index(field)]
    return (GLB_S if end == "lb" else GUB_S)[synth.STATE_NAMES.index(field)]


_shared = {}


def _base(structure, n):
    """Mesh, forcing and observations shared by the cases of one structure and mesh size."""
    if (structure, n) not in _shared:
        from oracle import pyoracle
        m = synth.make_mesh(n, n, ng=2)
        prcp, pet = synth.dense_forcing(m, NT, gap_per_million=GAPS)
        Pq = synth.make_parameters(n, n, perturb=0.1)
        S = synth.make_states(n, n, warm=True)
        qobs = pyoracle.run(structure, m, DT, prcp, pet, np.zeros((m.ng, NT), np.float32), Pq, S)["qsim"].copy()
        _shared[structure, n] = (m, prcp, pet, np.asfortranarray(qobs, np.float32))
    return _shared[structure, n]


def build(cid):
    """Case cid as the namespace test_gpu_parity._types reads (structure, dt, nt, mesh, prcp, pet, qobs, params, states, opts), plus
    .id and .direction (the params_d dict)."""
    kind, structure, *rest = cid.split(":")
    n = 12 if kind == "B" else 16
    m, prcp, pet, qobs = _base(structure, n)
    P = synth.make_parameters(n, n)
    S = synth.make_states(n, n, warm=True)
    if kind == "B":
        field, end = rest
        assert field in fields(structure) and end in ("lb", "ub"), cid
        (P if field in P else S)[field][:, ::2] = bound_value(field, end)
    else:
        assert kind == "O" and structure in OUTSIDE and not rest, cid
        rng = np.random.default_rng(11)
        if structure == "vic-a":
            mask = rng.random((n, n)) < 0.5
            for k, v in OUTSIDE_VIC:
                S[k][mask] = np.float32(v)
        else:
            for k, v in OUTSIDE_STATES:
                mask = rng.random((n, n)) < 0.5
                if k in gu.STRUCT_STATES[structure]:
                    S[k][mask] = np.float32(v)
    ps = gu.STRUCT_PARAMS[structure]
    d = {k: np.asfortranarray((np.float32(0.01) * P[k] if k in ps else np.zeros_like(P[k])).astype(np.float32)) for k in synth.PARAM_NAMES}
    return types.SimpleNamespace(id=cid, structure=structure, dt=DT, nt=NT, mesh=m, prcp=prcp, pet=pet, qobs=qobs, params=P, states=S,
                                 opts={}, direction=d)


def without_ci(g):
    """Case g with ci's plane of the composite direction zeroed.  The forcing's PET is exactly zero at night, which puts the
    interception operator of gr-b and gr-c on the kink of min(pet, prcp + hi ci) (tests/tangent_field_cases.py): along ci the fp32
    oracle is 5 .. 40 % away from the fp64 truth, and that noise lifts the composite direction's bar to 1e-4 .. 1e-3.  Without ci in
    the direction the bar is back at 3e-7 .. 5e-6."""
    d = dict(g.direction, ci=np.zeros_like(g.direction["ci"]))
    return types.SimpleNamespace(**dict(vars(g), id=g.id + " no-ci", direction=d))


def floor_copy(g):
    """Case g with every exactly zero PET value at tangent_field_cases.PET_FLOOR: off the interception kink."""
    import tangent_field_cases as tf
    return types.SimpleNamespace(**dict(vars(g), id=g.id + " floor", pet=tf.floor_pet(g.pet)))


def tangent_extras(g):
    """The tangent directions of case g beyond its composite one, each with the oracle's answers along it: a list of
    (label, case, (params_d, states_d), field, ref32, ref64, grad32, truth) where case is g or its floor copy, field the lone field
    of the direction (None: the composite direction without ci), ref32 / ref64 the dicts of tangent_field_cases.oracle_tangent,
    grad32 the fp32 oracle's gradient plane of field on a floor copy (None: the case's own adjoint outputs hold it) and truth whether
    the truth rule applies (the fp32 oracle within tangent_field_cases.E_REF_CAP of the fp64 truth on every gauge).
      * gr-b, gr-c, every case: the composite direction without ci (without_ci);
      * every B: case: tangent_field_cases.field_direction of the field on the bound, parameter or state.  It always takes the
        adjoint-tangent identity; the truth rule where truth;
      * the ci and hi cases of gr-b and gr-c: the same direction once more on the floor copy of the case, truth rule included."""
    import tangent_field_cases as tf
    kind, structure, *rest = g.id.split(":")
    zero_states = {k: np.zeros_like(v) for k, v in g.states.items()}
    out = []

    def add(label, case, direction, field, grad32=None):
        r32, r64 = tf.oracle_tangent(case, direction), tf.oracle_tangent(case, direction, fp64=True)
        out.append((label, case, direction, field, r32, r64, grad32, field is None or max(tf.e_ref(r32, r64)) <= tf.E_REF_CAP))

    if "ci" in gu.STRUCT_PARAMS[structure]:
        add(g.id + " no-ci", g, (without_ci(g).direction, zero_states), None)
    if kind == "B":
        field = rest[0]
        add(f"{g.id} lone {field}", g, tf.field_direction(g, field), field)
        if field in ("ci", "hi"):
            gf = floor_copy(g)
            add(f"{gf.id} lone {field}", gf, tf.field_direction(gf, field), field, grad32=tf.oracle_gradient(gf)[field])
            assert out[-1][-1], (gf.id, tf.e_ref(*out[-1][4:6]))
    return out


def oracle_outputs(g, fp64=False, kinds=("fwd", "adj", "tan")):
    """The oracle's outputs of case g in fp32 or fp64 as a flat dict of float64 arrays, under the keys of size_cases.oracle_outputs:
    qsim, cost, fstates.<k> (forward); adj.qsim, adj.cost, <k>_b (adjoint); qsim_d, cost_d, tan.qsim (tangent).  With "fwd" in kinds
    also returns the branch census of the forward run; (outputs, census or None)."""
    from oracle import pyoracle
    ps, ss = gu.STRUCT_PARAMS[g.structure], gu.STRUCT_STATES[g.structure]
    a = (g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
    out, census = {}, None
    if "fwd" in kinds:
        f = pyoracle.run(*a, fp64=fp64, **g.opts)
        census = pyoracle.census(fp64)
        out["qsim"], out["cost"] = f["qsim"], f["cost"]
        out.update({"fstates." + k: f["fstates"][k] for k in ss})
    if "adj" in kinds:
        b = pyoracle.run(*a, adjoint=True, fp64=fp64, **g.opts)
        out["adj.qsim"], out["adj.cost"] = b["qsim"], b["cost"]
        out.update({k + "_b": b["parameters_b"][k] for k in ps})
        out.update({k + "_b": b["states_b"][k] for k in ss})
    if "tan" in kinds:
        t = pyoracle.run(*a, params_d=g.direction, fp64=fp64, **g.opts)
        out["qsim_d"], out["cost_d"], out["tan.qsim"] = t["qsim_d"], t["cost_d"], t["qsim"]
    return {k: np.asarray(v, np.float64) for k, v in out.items()}, census
