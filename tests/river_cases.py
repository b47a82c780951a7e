"""River trees shaped to stress the routing tables and the chained launches, and their CPU-oracle outputs, for
tests/test_river_cases_cpu.py and tests/test_gpu_river_cases.py.  A plain helper module like size_cases.py: every case is rebuilt
from its id alone through synth.Mesh, synth.make_path and synth.pick_gauges (two gauges), dx = 1000 m, dt = 3600 s,
synth.dense_forcing with 2 % data gaps, make_parameters and warm make_states; observations are the fp32 oracle's discharge at
parameters + 10 %, as size_cases.build makes them.

D8 codes 1..8 = N, NE, E, SE, S, SW, W, NW.  The builders:

  snake(nrow, ncol)     one serpentine chain through every cell: even rows run E, odd rows W, the last cell of a row runs S.
  comb(nrow, ncol)      every column flows S into a last row that flows E: every stem cell has two children, the stem and a column.
  fans(strips, blocks, out, drop)
                        chains of 3 x 3 blocks along code `out`.  The neighbour of a centre at -D[k] carries code k + 1 and so drains
                        into the centre; the centre leaves by `out`, its receiver carries `out` too and lands on the neighbour of the
                        next centre, which also carries `out`.  Seven children at every centre, none of them a basin outlet except
                        the last.  out = 1, 3, 5, 7: the chain runs N, E, S, W (the same plane rotated), `strips` chains side by
                        side, each a basin of its own.  out = 4: one chain along the diagonal, blocks stepping (3, 3), the rest of
                        the square masked.  drop: D8 positions 1..8 around every centre (position p = the neighbour at +D[p - 1])
                        that are masked (inactive, -99), so that the fan-in becomes 6, 5 or 4 with holes at chosen positions and the
                        active mask ragged.  Position `out` is the receiver and may not be dropped; the position opposite to `out`
                        is the link from the block before, and dropping it cuts the chain into one small basin per block.
  fan8(n)               n x n blocks of 3 x 3 whose centres carry code 0: outlets that point nowhere, the only way eight neighbours
                        can drain into one cell without a pit pair.  Fan-in 8 therefore occurs only at roots.
  singles(nrow, ncol)   active cells on the even / even lattice only: one-cell basins, no routing edge at all.

synth.flow_accumulation counts a cell with code 0 as nothing, so the one builder that has such cells (fan8) accumulates with a walk
down every path; the kernels read flwacc > 1.

PLAN holds, per mesh and group size, what the schedule builder (smash_amd/csrc/sx_plan.cpp, one level per super-step) makes of it:
(rounds, groups, series, deepest).  tests/test_river_cases_cpu.py holds the table to tests/csrc/sx_plan_check, the GPU tests hold
smashx_get_timing to the table."""
from __future__ import annotations

import types

import numpy as np

from smash_amd import synth

DT = 3600.0
DX = 1000.0
GAPS = 20000
DROW = (-1, -1, 0, 1, 1, 1, 0, -1)
DCOL = (0, 1, 1, 1, 0, -1, -1, -1)
DIRECTION = ("cp", "cft", "lr")


# ---- builders: flow-direction planes, -99 where inactive ---------------------------------------------------------------------------------------------------
def snake(nrow, ncol):
    fd = np.zeros((nrow, ncol), np.int32)
    fd[0::2, :] = 3
    fd[1::2, :] = 7
    fd[0::2, ncol - 1] = 5
    fd[1::2, 0] = 5
    return fd


def comb(nrow, ncol):
    fd = np.full((nrow, ncol), 5, np.int32)
    fd[nrow - 1, :] = 3
    return fd


def fans(strips, blocks, out=3, drop=()):
    assert out in (1, 3, 5, 7) or (out == 4 and strips == 1), out
    assert all(1 <= p <= 8 and p != out for p in drop), drop
    dr, dc = DROW[out - 1], DCOL[out - 1]
    pr, pc = (abs(dc), abs(dr)) if out != 4 else (0, 0)           # strips side by side, across the chain
    cells = {}
    for s in range(strips):
        for b in range(blocks):
            r0, c0 = 3 * b * dr + 3 * s * pr, 3 * b * dc + 3 * s * pc
            cells[(r0, c0)] = out
            for k in range(8):
                p = 1 + (k + 4) % 8                               # the neighbour at -D[k] stands at position p = the opposite of k + 1
                if p in drop:
                    continue
                cells[(r0 - DROW[k], c0 - DCOL[k])] = out if p == out else k + 1
    rmin, cmin = min(r for r, _ in cells), min(c for _, c in cells)
    n = 3 * blocks
    shape = (n, n) if out == 4 else (3 * strips, n) if out in (3, 7) else (n, 3 * strips)
    fd = np.full(shape, -99, np.int32)
    for (r, c), v in cells.items():
        fd[r - rmin, c - cmin] = v
    return fd


def fan8(n):
    fd = np.zeros((3 * n, 3 * n), np.int32)
    for k in range(8):
        fd[1 - DROW[k]::3, 1 - DCOL[k]::3] = k + 1
    return fd


def singles(nrow, ncol):
    fd = np.full((nrow, ncol), -99, np.int32)
    fd[0::2, 0::2] = 5
    return fd


BUILDERS = dict(snake=snake, comb=comb, fans=fans, fan8=fan8, singles=singles)


def _walk_accumulation(fd, active):
    nrow, ncol = fd.shape
    acc = np.where(active == 1, 0, -99).astype(np.int32)
    for r in range(nrow):
        for c in range(ncol):
            rr, cc = r, c
            while 0 <= rr < nrow and 0 <= cc < ncol and active[rr, cc] == 1:        # every cell counts on its whole path down
                acc[rr, cc] += 1
                d = fd[rr, cc]
                if d < 1:
                    break
                rr, cc = rr + DROW[d - 1], cc + DCOL[d - 1]
    return acc


_meshes = {}


def mesh_of(key):
    """synth.Mesh of a mesh key (builder name, args, sorted kwargs items); built once."""
    if key not in _meshes:
        fn, args, kw = key
        fd = np.asarray(BUILDERS[fn](*args, **dict(kw)), np.int32)
        active = (fd >= 0).astype(np.int32)
        if np.any(fd == 0):
            acc = _walk_accumulation(fd, active)
        else:
            acc = np.asarray(synth.flow_accumulation(np.asfortranarray(fd), np.asfortranarray(active)))
        gauges = synth.pick_gauges(np.where(active == 1, acc, -1), 2)
        area = np.array([float(acc[r, c]) * DX * DX for r, c in gauges], np.float32)
        nrow, ncol = fd.shape
        _meshes[key] = synth.Mesh(nrow, ncol, DX, fd, acc, synth.make_path(acc), active, gauges, area)
    return _meshes[key]


def upstream(m):
    """(fan-in histogram over 0..8 children, longest path in edges) of the active cells of mesh m.  A cell with code 0 or one that
    points off the plane or at an inactive cell has no receiver."""
    fd, act = np.asarray(m.flwdir), np.asarray(m.active_cell)
    nrow, ncol = fd.shape
    down, fanin = {}, {}
    for r in range(nrow):
        for c in range(ncol):
            if act[r, c] != 1:
                continue
            fanin.setdefault((r, c), 0)
            d = fd[r, c]
            if d < 1:
                continue
            rr, cc = r + DROW[d - 1], c + DCOL[d - 1]
            if 0 <= rr < nrow and 0 <= cc < ncol and act[rr, cc] == 1:
                down[(r, c)] = (rr, cc)
                fanin[(rr, cc)] = fanin.get((rr, cc), 0) + 1
    hist = [0] * 9
    for v in fanin.values():
        hist[v] += 1
    height = {}
    for cell in sorted(fanin, key=lambda q: m.flwacc[q]):                  # ascending accumulation: children before their receiver
        height.setdefault(cell, 0)
        if cell in down:
            height[down[cell]] = max(height.get(down[cell], 0), height[cell] + 1)
    return hist, max(height.values())


# ---- meshes, their shape and what the schedule builder makes of them ----------------------------------------------------------------------
def _key(fn, *args, **kw):
    return (fn, args, tuple(sorted(kw.items())))


SNAKE_S, SNAKE_L = _key("snake", 16, 24), _key("snake", 33, 40)
COMB = _key("comb", 9, 80)
FANS = {out: _key("fans", 1, 40, out=out) for out in (1, 3, 4, 5, 7)}
DROPS = ((1,), (8,), (2, 5), (1, 4, 7))
FANS_DROP = {d: _key("fans", 2, 20, drop=d) for d in DROPS}
FOREST = _key("fans", 4, 12)
FAN8 = _key("fan8", 3)
SINGLES = _key("singles", 21, 23)

# mesh key -> (cells, fan-in histogram, longest path)
SHAPE = {
    SNAKE_S: (384, [1, 383, 0, 0, 0, 0, 0, 0, 0], 383),
    SNAKE_L: (1320, [1, 1319, 0, 0, 0, 0, 0, 0, 0], 1319),
    COMB: (720, [80, 561, 79, 0, 0, 0, 0, 0, 0], 87),
    FOREST: (432, [292, 92, 0, 0, 0, 0, 0, 48, 0], 35),
    FAN8: (81, [72, 0, 0, 0, 0, 0, 0, 0, 9], 1),
    SINGLES: (132, [132, 0, 0, 0, 0, 0, 0, 0, 0], 0),
    FANS_DROP[(1,)]: (320, [202, 78, 0, 0, 0, 0, 40, 0, 0], 59),
    FANS_DROP[(8,)]: (320, [202, 78, 0, 0, 0, 0, 40, 0, 0], 59),
    FANS_DROP[(2, 5)]: (280, [162, 78, 0, 0, 0, 40, 0, 0, 0], 59),
    FANS_DROP[(1, 4, 7)]: (240, [160, 40, 0, 0, 40, 0, 0, 0, 0], 2),
}
SHAPE.update({k: (360, [241, 79, 0, 0, 0, 0, 0, 40, 0], 119) for k in FANS.values()})

# (mesh key, group size) -> (rounds, groups, series, deepest)
PLAN = {
    (SNAKE_S, 64): (7, 7, 6, 63), (SNAKE_S, 512): (1, 1, 0, 383),
    (SNAKE_L, 64): (21, 21, 20, 63), (SNAKE_L, 512): (3, 3, 2, 511),
    (COMB, 64): (4, 14, 76, 31), (COMB, 512): (2, 3, 25, 63),
    (FANS_DROP[(1,)], 64): (3, 8, 124, 23), (FANS_DROP[(1,)], 512): (1, 1, 0, 59),
    (FANS_DROP[(8,)], 64): (3, 8, 124, 23), (FANS_DROP[(8,)], 512): (1, 1, 0, 59),
    (FANS_DROP[(2, 5)], 64): (3, 7, 92, 27), (FANS_DROP[(2, 5)], 512): (1, 1, 0, 59),
    (FANS_DROP[(1, 4, 7)], 64): (1, 4, 0, 2), (FANS_DROP[(1, 4, 7)], 512): (1, 1, 0, 2),
    (FOREST, 64): (2, 10, 124, 21), (FOREST, 512): (1, 1, 0, 35),
    (FAN8, 64): (1, 2, 0, 1), (FAN8, 512): (1, 1, 0, 1),
    (SINGLES, 64): (1, 3, 0, 0), (SINGLES, 512): (1, 2, 0, 0),
}
for _k in FANS.values():                                      # the same tree under every rotation
    PLAN[(_k, 64)], PLAN[(_k, 512)] = (6, 10, 203, 21), (1, 1, 0, 119)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def _case(mesh, nt, group, structure="gr-b"):
    return dict(mesh=mesh, nt=nt, group=group, structure=structure)


CASES = {"S1": _case(SNAKE_S, 96, 64), "S2": _case(SNAKE_L, 260, 512)}
CASES.update({f"S3-nt{nt}": _case(SNAKE_S, nt, 64) for nt in (3, 5, 255, 256, 257, 516)})
CASES.update({"C1": _case(COMB, 48, 64), "F1": _case(FANS[3], 48, 64)})
CASES.update({f"F2-out{out}-g{g}": _case(FANS[out], 48, g) for out in (1, 5, 7, 4) for g in (64, 512)})
CASES.update({"F3-drop" + "".join(map(str, d)): _case(FANS_DROP[d], 48, 64) for d in DROPS})
CASES.update({"F4-vic-a": _case(FOREST, 48, 64, "vic-a"), "F4-gr-d": _case(FOREST, 48, 64, "gr-d")})
CASES.update({"E1": _case(FAN8, 48, 64), "N1": _case(SINGLES, 23, 64)})


def problem(cid):
    """What the oracle's answer depends on: cases that differ in the group size alone share it."""
    c = CASES[cid]
    return c["mesh"], c["nt"], c["structure"]


_built = {}


def build(cid):
    """Case cid as the namespace test_gpu_parity._types reads (structure, dt, nt, mesh, prcp, pet, qobs, params, states, opts), plus
    .id, .group and .direction (the tangent direction: 1 % of cp, cft and lr).  Built once per problem; the arrays are shared."""
    from oracle import pyoracle
    key = problem(cid)
    if key not in _built:
        mk, nt, structure = key
        m = mesh_of(mk)
        prcp, pet = synth.dense_forcing(m, nt, gap_per_million=GAPS)
        P = synth.make_parameters(m.nrow, m.ncol)
        S = synth.make_states(m.nrow, m.ncol, warm=True)
        Pq = synth.make_parameters(m.nrow, m.ncol, perturb=0.1)
        qobs = pyoracle.run(structure, m, DT, prcp, pet, np.zeros((m.ng, nt), np.float32), Pq, S)["qsim"].copy()
        d = {k: np.asfortranarray((np.float32(0.01) * P[k] if k in DIRECTION else np.zeros_like(P[k])).astype(np.float32))
             for k in synth.PARAM_NAMES}
        _built[key] = dict(structure=structure, dt=DT, nt=nt, mesh=m, prcp=prcp, pet=pet, qobs=np.asfortranarray(qobs, np.float32),
                           params=P, states=S, opts={}, direction=d)
    return types.SimpleNamespace(id=cid, group=CASES[cid]["group"], **_built[key])


_oracle = {}


def oracle_outputs(cid, fp64=False):
    """The oracle's outputs of case cid in fp32 or fp64, as size_cases.oracle_outputs lays them out: qsim, cost, fstates.<k>
    (forward); adj.qsim, adj.cost, <k>_b (adjoint); qsim_d, cost_d, tan.qsim (tangent).  Computed once per problem, read-only."""
    import golden_util as gu
    from oracle import pyoracle
    key = problem(cid) + (bool(fp64),)
    if key not in _oracle:
        g = build(cid)
        ps, ss = gu.STRUCT_PARAMS[g.structure], gu.STRUCT_STATES[g.structure]
        a = (g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states)
        out = {}
        f = pyoracle.run(*a, fp64=fp64)
        out["qsim"], out["cost"] = f["qsim"], f["cost"]
        out.update({"fstates." + k: f["fstates"][k] for k in ss})
        b = pyoracle.run(*a, adjoint=True, fp64=fp64)
        out["adj.qsim"], out["adj.cost"] = b["qsim"], b["cost"]
        out.update({k + "_b": b["parameters_b"][k] for k in ps})
        out.update({k + "_b": b["states_b"][k] for k in ss})
        t = pyoracle.run(*a, params_d=g.direction, fp64=fp64)
        out["qsim_d"], out["cost_d"], out["tan.qsim"] = t["qsim_d"], t["cost_d"], t["qsim"]
        out = {k: np.asarray(v, np.float64) for k, v in out.items()}
        for v in out.values():
            v.setflags(write=False)
        _oracle[key] = out
    return _oracle[key]


def reference(cid):
    """{False: fp32 outputs, True: fp64 outputs} of case cid, the second half of what size_cases.oracle_all gives per case."""
    return {False: oracle_outputs(cid, False), True: oracle_outputs(cid, True)}
