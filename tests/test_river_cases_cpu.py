"""CPU: the constructed river trees of tests/river_cases.py.  Their shape (cells, upstream fan-in, longest path) and what the
schedule builder makes of them at groups of 64 and 512 are the numbers the case table quotes; the C oracle is bit-identical to the
compiled reference on them, forward and adjoint (skipped where oracle/_ref is not built); and the fp32 oracle itself is within 1e-3
of the fp64 statements on every output the GPU tests assert, so that the default-build bar of tests/test_gpu_river_cases.py
(e_hip <= 2 e_ref + 1e-6) cannot go slack on an ill-conditioned case."""
import numpy as np
import pytest

import golden_util as gu
import river_cases as rc
from test_plan_sanitized import _run, exe  # noqa: F401  (the module fixture that builds tests/csrc/sx_plan_check with ASan + UBSan)

MESHES = {}
for _cid, _c in rc.CASES.items():
    MESHES.setdefault(_c["mesh"], _cid)
MESH_IDS = [f"{k[0]}{'x'.join(map(str, k[1]))}" + "".join(f"-{a}{v}" for a, v in k[2]).replace(" ", "") for k in MESHES]
E_REF_MAX = 1e-3
SCALAR = ("cost", "adj.cost", "cost_d")


@pytest.mark.parametrize("key", list(MESHES), ids=MESH_IDS)
def test_shape_of_every_mesh(key):
    m = rc.mesh_of(key)
    hist, longest = rc.upstream(m)
    print(key, "cells", m.nac, "fan-in", hist, "longest path", longest)
    assert (m.nac, hist, longest) == rc.SHAPE[key]
    assert m.ng == 2 and np.all(np.asarray(m.active_cell)[m.gauge_pos[:, 0], m.gauge_pos[:, 1]] == 1)
    assert np.array_equal(np.asarray(m.flwacc) >= 1, np.asarray(m.active_cell) == 1)


def test_fans_drop_masks_the_named_positions():
    """position p of drop is the neighbour at +D[p - 1] of every centre; the other neighbours stay and still drain into the centre"""
    for d in rc.DROPS:
        m = rc.mesh_of(rc.FANS_DROP[d])
        act, fd = np.asarray(m.active_cell), np.asarray(m.flwdir)
        for r0 in (1, 4):
            for c0 in range(1, 60, 3):
                for p in range(1, 9):
                    r, c = r0 + rc.DROW[p - 1], c0 + rc.DCOL[p - 1]
                    assert (act[r, c] == 0) == (p in d), (d, r0, c0, p)
                    if p not in d and p != 3:
                        assert (r + rc.DROW[fd[r, c] - 1], c + rc.DCOL[fd[r, c] - 1]) == (r0, c0)


@pytest.mark.parametrize("group", [64, 512])
@pytest.mark.parametrize("key", list(MESHES), ids=MESH_IDS)
def test_schedule_of_every_mesh(exe, key, group):  # noqa: F811
    m = rc.mesh_of(key)
    out = _run(exe, m, group, sublevels=1)
    print(key, group, out)
    assert out.startswith(f"ok cells {m.nac} ")
    w = out.split()
    got = tuple(int(w[w.index(k) + 1]) for k in ("rounds", "groups", "series", "deepest"))
    assert got == rc.PLAN[(key, group)]


def test_the_table_reaches_what_it_says():
    """a group as deep as it is large less one; steps below a group's depth; chained rounds by the plan's own rule (three rounds)"""
    assert rc.PLAN[(rc.SNAKE_L, 512)][3] == 511 and rc.PLAN[(rc.SNAKE_S, 64)][3] == 63
    assert rc.CASES["S3-nt3"]["nt"] < 63 and rc.CASES["S3-nt5"]["nt"] < 63
    for cid in ("S1", "S2", "S3-nt255", "S3-nt256", "S3-nt257", "S3-nt516", "F1", "C1"):
        c = rc.CASES[cid]
        assert rc.PLAN[(c["mesh"], c["group"])][0] >= 3, cid
    for cid, c in rc.CASES.items():
        assert (c["mesh"], c["group"]) in rc.PLAN, cid


@pytest.mark.parametrize("cid", ["S1", "C1", "F1", "F3-drop25", "E1"])
def test_oracle_is_bit_identical_to_the_reference(cid):
    from oracle import pyoracle, refbind
    if not refbind.available():
        pytest.skip("oracle/_ref/libsmash_ref.so not built (needs the reference's sources and flang)")
    g = rc.build(cid)
    a = (g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
    ref = refbind.run(*a, adjoint=True)
    orc = pyoracle.run(*a, adjoint=True)
    assert np.all(np.isfinite(ref["qsim"])) and float(np.max(ref["qsim"])) > 0.0
    assert np.array_equal(ref["qsim"], orc["qsim"]) and np.float32(ref["cost"]) == np.float32(orc["cost"])
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(ref["parameters_b"][k], orc["parameters_b"][k]), k
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(ref["states_b"][k], orc["states_b"][k]), k
    fwd = refbind.run(*a)
    assert np.array_equal(fwd["qsim"], rc.oracle_outputs(cid)["qsim"].astype(np.float32))


PROBLEMS = {}
for _cid in rc.CASES:
    PROBLEMS.setdefault(rc.problem(_cid), _cid)


def _ill_conditioned(cid):
    """The outputs on which the fp32 oracle itself is farther than E_REF_MAX from the fp64 statements, pinned so that the list cannot
    grow silently.  Measured (this test prints every figure):
      * ci_b and hi_b of every gr-b case, 5e-2 (F2-out1) ... 7.7e-1 (E1), 1.0 on N1: the interception fields of gr-b are ill-conditioned
        in fp32 (7e-2 at 512^2 x 160); no forcing seed of 1 ... 45 brings them under the bound on all cases at once.
      * cp_b of the three- and five-step runs (7.3e-3, 4.7e-3) and cp_b, hp_b of the 23 steps of one-cell basins (1.0, 0.99): the
        production store has hardly moved, its gradient is a rounding residue (N1: 1e-18 against 1e-14).
    On these the default-build bar of the GPU tests (2 e_ref + 1e-6) is a sanity bar only; what holds them is bit-identity with the
    oracle in the exact-libm build.  Every other output of every case meets the bound, E1's cp_b at the table's nt = 48 (4.1e-4)."""
    ill = {"ci_b", "hi_b"} if rc.CASES[cid]["structure"] == "gr-b" else set()
    return ill | {"S3-nt3": {"cp_b"}, "S3-nt5": {"cp_b"}, "N1": {"cp_b", "hp_b"}}.get(cid, set())


@pytest.mark.parametrize("cid", list(PROBLEMS.values()))
def test_the_reference_alone_is_well_conditioned(cid):
    """e_ref = rel_l2(oracle32, oracle64) <= 1e-3 on every asserted output (discharge per gauge, final states, every gradient field,
    the tangent discharge); the costs are finite and the fp32 one is within 1e-3 of the fp64 one, relative.  The outputs over the
    bound are exactly the pinned ones of _ill_conditioned."""
    o32, o64 = rc.oracle_outputs(cid, False), rc.oracle_outputs(cid, True)
    worst = {}
    for k, v in o32.items():
        t = o64[k]
        if k in SCALAR:
            e = abs(float(v) - float(t)) / max(abs(float(t)), 1e-30)
        elif k in ("qsim", "adj.qsim", "qsim_d", "tan.qsim"):
            e = max(gu.rel_l2(v[i], t[i]) for i in range(v.shape[0]))
        else:
            e = gu.rel_l2(v, t)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(t)), k
        worst[k] = e
    print(cid, " ".join(f"{k} {e:.1e}" for k, e in worst.items()))
    bad = {k: e for k, e in worst.items() if not e <= E_REF_MAX}
    assert set(bad) == _ill_conditioned(cid), (cid, bad)
