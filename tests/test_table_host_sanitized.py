"""CPU: the host tables of the sample paths and the forcing statistics (smash_amd/csrc/sx_tablehost.h: the river forest, the per-thread
tables of the catchment-resident kernel, the catchment lists, the index lists) in a stand-alone program
(tests/csrc/sx_tablehost_check.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer, every input a heap block of exactly its
size.  The program verifies the tables' invariants; this file compares what it prints, exactly and floats by their bits, with the
restatements pinned to the reference's fixtures (mean_forcing_util.upstream, prcp_indices_util.gauge_tables) and checks the words of
every refusal.  The device side runs under no sanitizer; tests/test_gpu_mean_forcing.py, tests/test_gpu_prcp_indices.py,
tests/test_gpu_ensemble.py and tests/test_gpu_uniform_costs.py cover its results."""
import copy
import os
import subprocess
import time

import numpy as np
import pytest

import golden_util as gu
import mean_forcing_util as mu
import prcp_indices_util as pu
from smash_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "smash_amd", "csrc")
EXE = os.path.join(HERE, "csrc", "sx_tablehost_check")
F = np.float32
MAXCELLS = 1024                     # SX_RES_MAXCELLS
CYCLE = "flow directions contain a cycle over active cells"


@pytest.fixture(scope="module")
def exe():
    src = [os.path.join(HERE, "csrc", "sx_tablehost_check.cpp"), os.path.join(CSRC, "sx_plan.cpp")]
    deps = src + [os.path.join(CSRC, f) for f in ("sx_tablehost.h", "sx_tables.h", "sx_plan.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", EXE] + src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return EXE


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32).astype(np.int64)


def _run(exe, m, flwdst=None, lds=None):
    """the checker on mesh m -> {name: int64 array | refusal text, "pi_gauge": [rows]}; floats stay bit patterns"""
    flat = lambda a: " ".join(map(str, np.asarray(a, np.int64).reshape(-1, order="F")))      # noqa: E731
    txt = f"{m.nrow} {m.ncol}\n{flat(m.flwdir)}\n{flat(m.active_cell)}\n{m.ng}\n{flat(m.gauge_pos)}\n"
    if flwdst is not None:
        txt += "flwdst " + " ".join(map(str, _bits(np.asarray(flwdst, F).reshape(-1, order="F")))) + "\n"
    if lds is not None:
        txt += f"lds {lds[0]} {lds[1]}\n"
    t0 = time.perf_counter()
    r = subprocess.run([exe], input=txt, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    wall = time.perf_counter() - t0
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "VIOLATION" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-1500:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok", lines[-1][:200]
    out = {"pi_gauge": [], "wall": wall}
    for line in lines[:-1]:
        name, _, rest = line.partition(" ")
        if name.endswith("_refusal"):
            out[name] = rest
        elif name == "pi_gauge":
            out[name].append(np.array(rest.split(), np.int64))
        else:
            out[name] = np.array(rest.split(), np.int64)
    return out


def _with(m, **changes):
    """a copy of mesh m with some fields replaced"""
    m = copy.copy(m)
    for k, v in changes.items():
        setattr(m, k, np.asfortranarray(v, dtype=np.int32))
    m.ng = int(np.asarray(m.gauge_pos).reshape(-1, 2).shape[0])
    return m


def _k_of(m, out):
    kof = np.full(m.nrow * m.ncol, -1, np.int64)
    kof[out["cell_flat"]] = np.arange(out["cell_flat"].size)
    return kof.reshape(m.nrow, m.ncol, order="F")


def _pad64(parts, fill=-1):
    """the parts one after the other, each filled up to a whole number of blocks of 64"""
    return np.concatenate([np.concatenate([np.asarray(p, np.int64), np.full(-len(p) % 64, fill, np.int64)]) for p in parts] or [np.zeros(0, np.int64)])


def _upstream_lists(m, out):
    """up (n, 8), upn: one step of mean_forcing_util.upstream's neighbour rule, over the plan's cells, in ascending D8 code"""
    kof = _k_of(m, out)
    n = out["cell_flat"].size
    r, c = out["cell_flat"] % m.nrow, out["cell_flat"] // m.nrow
    up, upn = np.full((n, 8), -1, np.int64), np.zeros(n, np.int64)
    for i in range(8):
        rn, cn = r + mu.DROW[i], c + mu.DCOL[i]
        ok = (rn >= 0) & (rn < m.nrow) & (cn >= 0) & (cn < m.ncol)
        rn, cn = np.where(ok, rn, 0), np.where(ok, cn, 0)
        hit = ok & (np.asarray(m.flwdir)[rn, cn] == i + 1) & (kof[rn, cn] >= 0)
        up[hit, upn[hit]] = kof[rn, cn][hit]
        upn += hit
    return up, upn


def _eight():
    """8 x 8, three gauges: the outlet, an interior cell, and the outlet again"""
    m = synth.make_mesh(8, 8, ng=2)
    gp = np.asarray(m.gauge_pos)
    return _with(m, gauge_pos=np.array([gp[0], gp[1], gp[0]]))


def _france():
    """the two largest basins of the raster of France; two gauges on rows whose (row, row) cell is active, as the index tables ask"""
    m = synth.make_mesh_france(2, ng=2)
    act = np.asarray(m.active_cell) == 1
    rows = np.arange(m.nrow)
    diag = (rows < m.ncol) & act[rows, np.minimum(rows, m.ncol - 1)]
    return _with(m, gauge_pos=synth.pick_gauges(np.where(act & diag[:, None], m.flwacc, -1), 2))


@pytest.fixture(scope="module")
def runs(exe):
    """(label, mesh, flwdst, tables) of every input, each run once"""
    inputs = []
    assert set(mu.CASES.values()) <= set(pu.CASES.values())
    for name in sorted(pu.CASES):
        inputs.append((name, gu.load(pu.CASES[name]).mesh, np.load(os.path.join(pu.DIR, name + ".npz"))["flwdst"]))
    for label, m in [("france", _france()), ("d8 seed 3", synth.make_mesh_d8(60, 72, ng=2, seed=3)),
                     ("d8 seed 11", synth.make_mesh_d8(60, 72, ng=2, seed=11)), ("corner", synth.make_mesh(64, 64, ng=1, mask_corner=True)),
                     ("8 x 8", _eight())]:
        inputs.append((label, m, synth.flow_distance(m.flwdir, m.active_cell, m.dx)))
    return [(label, m, fd, _run(exe, m, fd)) for label, m, fd in inputs]


def test_forest_equals_the_upstream_rule(runs):
    shown = set()
    for label, m, _, out in runs:
        n = out["cell_flat"].size
        assert n == m.nac, label
        up, upn = _upstream_lists(m, out)
        assert np.array_equal(out["upn"], upn) and np.array_equal(out["up"].reshape(n, 8), up), label
        if upn.max() >= 3:
            shown.add("a cell with three upstream cells")
        if np.count_nonzero(out["parent"] == -1) > 1:
            shown.add("more than one root")
        if "res_refusal" in out:
            assert n > MAXCELLS and out["res_refusal"] == f"{n} active cells, the resident kernel holds one cell per thread and at most {MAXCELLS}", label
            shown.add("more cells than the resident kernel holds")
            continue
        assert n <= MAXCELLS, label
        own = out["res_ownline"]
        if np.any((own != -1) & ((own & 31) >= 2)):
            shown.add("a delay line of four slots or more")
        if np.any(out["res_gnext"] != -1):
            assert np.unique(out["gauge_k"]).size < m.ng, label
            shown.add("two gauges on one cell")
    assert shown == {"a cell with three upstream cells", "more than one root", "more cells than the resident kernel holds",
                     "a delay line of four slots or more", "two gauges on one cell"}


def test_catchment_lists_equal_mask_upstream_cells(runs):
    longer = shorter = 0
    for label, m, _, out in runs:
        kof = _k_of(m, out)
        lists = []
        for r, c in np.asarray(m.gauge_pos).reshape(-1, 2):
            cols, rows = np.nonzero(mu.upstream(m.flwdir, r, c).T)
            lists.append(kof[rows, cols])
        assert np.array_equal(out["mf_count"], [len(x) for x in lists]), label
        assert np.array_equal(out["mf_begin"], np.cumsum([0] + [len(x) + (-len(x) % 64) for x in lists])), label
        assert np.array_equal(out["mf_list"], _pad64(lists)), label
        longer += int(np.count_nonzero(out["mf_count"] > 64))
        shorter += int(np.count_nonzero(out["mf_count"] < 64))
    assert longer > 0 and shorter > 0


def test_index_tables_equal_the_restatement(runs):
    outside = 0
    for label, m, flwdst, out in runs:
        kof = _k_of(m, out)
        tabs = pu.gauge_tables(m.flwdir, m.gauge_pos, flwdst)
        assert len(out["pi_gauge"]) == m.ng == len(tabs), (label, out.get("pi_refusal"))
        want_list, want_dl, want_d2l = [], [], []
        for g, (T, G) in enumerate(zip(tabs, out["pi_gauge"])):
            lb, db, krr, sec, wf, cnt = G[0], G[1], G[2], G[3:15], G[15:26], G[26:37]
            catch = kof[T["rows"], T["cols"]]
            bins = [kof[br, bc] for br, bc in T["bins"]]
            assert lb == sum(map(len, want_list)) and db == sum(map(len, want_dl)), (label, g)
            assert krr == kof[T["row"], T["row"]], (label, g)
            assert np.array_equal(wf, _bits(T["wf"])), (label, g)
            assert np.array_equal(cnt, _bits(np.array([0] + [len(b) for b in bins], F))), (label, g)
            assert np.array_equal(sec, np.cumsum([0] + [(len(x) + 63) // 64 for x in [catch] + bins])), (label, g)
            want_list.append(_pad64([catch] + bins))
            want_dl.append(_pad64([_bits(T["d"])], 0))
            want_d2l.append(_pad64([_bits(T["d"] * T["d"])], 0))
            if any(np.setdiff1d(b, catch).size for b in bins):
                outside += 1
        assert np.array_equal(out["pi_list"], np.concatenate(want_list)), label
        assert np.array_equal(out["pi_dl"], np.concatenate(want_dl)) and np.array_equal(out["pi_d2l"], np.concatenate(want_d2l)), label
    assert outside > 0                                  # a distance bin holds a cell outside the catchment


def test_france_wall_time(runs):
    """no bar: the figure for the record (the algorithms are the driver's own, moved)"""
    print("sx_tablehost_check on the France mesh: %.2f s" % dict((r[0], r[3]["wall"]) for r in runs)["france"])


def _comb(nrow, ncol, gauge):
    """every cell drains south, the last row east and its last cell off the grid: the catchment of (r, c) above the last row is the
    column c down to r"""
    fd = np.full((nrow, ncol), 5, np.int32)
    fd[nrow - 1, :] = 3
    fd[nrow - 1, ncol - 1] = 5
    return _with(synth.make_mesh(nrow, ncol, ng=1), flwdir=fd, gauge_pos=np.array([gauge]))


def test_refusals(exe):
    m = _comb(8, 8, (5, 2))
    assert np.count_nonzero(mu.upstream(m.flwdir, 5, 2)) == 6
    fd0 = synth.flow_distance(m.flwdir, m.active_cell, m.dx)
    # a two-cell cycle
    fd = np.asarray(m.flwdir).copy(order="F")
    fd[3, 3], fd[3, 4] = 3, 7                                    # E <-> W
    assert _run(exe, _with(m, flwdir=fd)).get("forest_refusal") == CYCLE
    # a catchment that runs into an inactive cell: a leaf of the gauge's catchment is made inactive and keeps its code
    mask = mu.upstream(m.flwdir, 5, 2)
    leaves = [(r, c) for r, c in zip(*np.nonzero(mask)) if np.count_nonzero(mu.upstream(m.flwdir, r, c)) == 1 and (r, c) != (5, 2)]
    r, c = leaves[0]
    act = np.asarray(m.active_cell).copy(order="F")
    act[r, c] = 0
    assert _run(exe, _with(m, active_cell=act), fd0).get("mf_refusal") == \
        f"smashx_mean_forcing: the catchment of gauge 0 contains the inactive cell ({r}, {c}): the plan holds no forcing there"
    # a one-cell catchment
    out = _run(exe, _with(m, gauge_pos=np.array([[r, c]])), fd0)
    assert out["mf_count"].tolist() == [1]
    assert out.get("pi_refusal") == "smashx_prcp_indices: the catchment of gauge 0 has 1 cell: the reference's quantile reads two"
    # (gauge_row, gauge_row) inactive, and in no catchment
    act = np.asarray(m.active_cell).copy(order="F")
    act[5, 5] = 0
    fd = np.asarray(m.flwdir).copy(order="F")
    fd[5, 5] = -99
    assert _run(exe, _with(m, active_cell=act, flwdir=fd), fd0).get("pi_refusal") == \
        "smashx_prcp_indices: gauge 0: the reference reads the rain of the cell (gauge_row, gauge_row) = (5, 5), which is inactive: the plan holds no forcing there"
    # (gauge_row, gauge_row) outside the grid
    tall = _comb(12, 8, (10, 3))
    assert _run(exe, tall, synth.flow_distance(tall.flwdir, tall.active_cell, tall.dx)).get("pi_refusal") == \
        "smashx_prcp_indices: gauge 0: the reference reads the rain of the cell (gauge_row, gauge_row) = (10, 10), which is outside the grid"
    # an inactive cell in a distance bin: (0, 7), in no catchment, at the distance of a cell of the catchment
    act = np.asarray(m.active_cell).copy(order="F")
    act[0, 7] = 0
    fd = np.asarray(m.flwdir).copy(order="F")
    fd[0, 7] = -99
    T = pu.gauge_tables(m.flwdir, m.gauge_pos, fd0)[0]
    d = np.sort(T["d"])[1]
    assert d > 0
    k = int(np.flatnonzero((d > T["qtl"][:-1]) & (d <= T["qtl"][1:]))[0]) + 1
    fdst = np.asarray(fd0).copy(order="F")
    fdst[0, 7] = fdst[5, 2] + d
    assert F(fdst[0, 7] - fdst[5, 2]) == d
    assert _run(exe, _with(m, active_cell=act, flwdir=fd), fdst).get("pi_refusal") == \
        f"smashx_prcp_indices: the inactive cell (0, 7) lies in distance bin {k} of gauge 0: the plan holds no forcing there"
    # an LDS limit of 64 B: the delay lines of 64 cells do not fit
    out = _run(exe, m, fd0, lds=(64, 16))
    need = out["res_refusal"].split(" need ")[1].split(" B of LDS")[0]
    assert int(need) > 64 and out["res_refusal"] == f"the delay lines of the catchment need {need} B of LDS, a workgroup may claim 64"
    fits = _run(exe, m, fd0)
    assert "res_refusal" not in fits and int(need) == 4 * int(fits["res_floats"][0]) + 16
