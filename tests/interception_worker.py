"""GPU steps of tests/test_gpu_interception.py, one per child process (python interception_worker.py <step>), so that every step
has a time limit of its own and the library build (SMASHX_EXACT_LIBM) is chosen per step.  Every comparison is exact equality of
fp32 bit patterns; each figure is printed before it is asserted."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import golden_util as gu            # noqa: E402
import interception_util as iu      # noqa: E402

SENTINEL = np.float32(-7.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sparse_order(m):
    """(rows, cols) of the active cells along mesh%path: the numbering of the (nac, nt) sparse vectors (mw_sparse_storage.f90:12-49)"""
    path, act = np.asarray(m.path), np.asarray(m.active_cell)
    keep = (path[0] >= 0) & (path[1] >= 0)
    keep[keep] &= act[path[0][keep], path[1][keep]] == 1
    return path[0][keep], path[1][keep]


def _plan(g, structure, prcp=None, pet=None, sparse=False, layout=None, tile=None, forcing=True):
    """a plan without gauges on the fixture's mesh (the routine reads the forcing and the active-cell mask, nothing else)"""
    import smash_amd
    from smash_amd.solver import Solver
    prcp, pet = (g.prcp if prcp is None else prcp), (g.pet if pet is None else pet)
    m = g.mesh
    setup = smash_amd.SetupDT(0, 0, structure=structure, dt=g.dt, ntime_step=g.nt, sparse_storage=sparse)
    mesh = smash_amd.MeshDT(setup, m.nrow, m.ncol, 0)
    mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.dx, m.flwdir, m.flwacc, m.path, m.active_cell
    mesh.gauge_pos, mesh.area = np.zeros((0, 2), np.int32, order="F"), np.zeros(0, np.float32)
    s = Solver(setup, mesh, tile=tile)
    if layout is not None:
        s.set_forcing_layout(**layout)
    if forcing:
        if sparse:
            rr, cc = _sparse_order(m)
            s.set_forcing(np.asfortranarray(prcp[rr, cc, :]), np.asfortranarray(pet[rr, cc, :]), sparse=True)
        else:
            s.set_forcing(prcp, pet)
    return s


def _check_plane(tag, got, want, act):
    nbad = int(np.sum(_bits(got[act]) != _bits(want[act])))
    nsent = int(np.sum(_bits(got[~act]) != _bits(np.full(int((~act).sum()), SENTINEL))))
    print(f"{tag}: {int(act.sum())} active cells, {np.unique(got[act]).size} distinct ci, {nbad} differ from the reference, "
          f"{nsent} inactive cells lost the sentinel", flush=True)
    assert nbad == 0 and nsent == 0, tag


def _structure(name, g):
    return g.structure if g.structure in ("gr-b", "gr-c") else "gr-b"         # Cance is a gr-a case: recorded, and run, as gr-b


def step_fixtures():
    """every fixture in every layout it admits against the reference's plane; inactive cells keep the sentinel"""
    from smash_amd import synth
    synth_layout = dict(compact=True, prcp_factor=0.1, pet_ratio=synth._pet_tables()[1], pet_hour0=0)
    for name in sorted(iu.CASES):
        g, day, nday, ci_ref = iu.load(name)
        act = np.asarray(g.mesh.active_cell) == 1
        st = _structure(name, g)
        layouts = [("dense", dict()), ("sparse", dict(sparse=True))]
        if "cance" in name:
            layouts.append(("compact-requested", dict(layout=dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1))))
        else:
            layouts.append(("compact", dict(layout=synth_layout)))
        for tag, kw in layouts:
            s = _plan(g, st, **kw)
            info = s.forcing_info()["layout"]
            if tag == "compact":
                assert info.startswith("compact"), info
            ci = np.full((g.mesh.nrow, g.mesh.ncol), SENTINEL, np.float32, order="F")
            out = s.adjust_interception(day, ci)
            assert out is ci
            _check_plane(f"{name} [{tag}: {info.split(':')[0]}]", ci, ci_ref, act)
            s.close()


def step_cance_compact():
    """Cance with both fields put on the fp32 reader's form (real(k) * 0.1, daily * ratio(hour) as float32 products: what the
    reference's reader produces), which loads into the compact layout; the yardstick on this forcing is the numpy restatement, and the
    fp32-rows plan on the same forcing must agree as well"""
    from smash_amd.solver import RATIO_PET_HOURLY as R
    g, day, nday, _ = iu.load("gr_a_cance_28x28x1440")
    prcp = np.asfortranarray(np.where(g.prcp < 0, g.prcp, np.rint(g.prcp / np.float32(0.1)).astype(np.float32) * np.float32(0.1)).astype(np.float32))
    pet = g.pet.copy(order="F")
    for d in range((g.nt + 1 + 23) // 24):
        ts = list(range(max(0, d * 24 - 1), min(g.nt, (d + 1) * 24 - 1)))
        tb = max(ts, key=lambda t: R[(t + 1) % 24])
        daily = (pet[:, :, tb] / R[(tb + 1) % 24]).astype(np.float32) if R[(tb + 1) % 24] > 0 else np.zeros(pet.shape[:2], np.float32)
        for t in ts:
            pet[:, :, t] = daily * R[(t + 1) % 24]
    act = np.asarray(g.mesh.active_cell) == 1
    rows, cols = np.nonzero(act)
    mine, _ = iu.adjust(prcp[rows, cols, :], pet[rows, cols, :], day)
    want = np.full(act.shape, SENTINEL, np.float32, order="F")
    want[rows, cols] = mine
    for tag, lay in (("compact", dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1)), ("fp32 rows", None)):
        s = _plan(g, "gr-b", prcp=prcp, pet=pet, layout=lay)
        info = s.forcing_info()["layout"]
        assert info.startswith(tag), info
        ci = np.full(act.shape, SENTINEL, np.float32, order="F")
        s.adjust_interception(day, ci)
        _check_plane(f"cance on the reader's form [{tag}] vs the numpy restatement", ci, want, act)
        s.close()


def step_tiles():
    """a 2 x 2 tiling: every part fills the cells it owns and nothing else; overlaid they give the single-domain plane"""
    from smash_amd import tiles
    for name in ("gr_c_32x32x240_d8_ragged", "gr_b_16x16x96_nse_gaps__start17"):
        g, day, nday, ci_ref = iu.load(name)
        act = np.asarray(g.mesh.active_cell) == 1
        pr, pc = tiles.tile_grid(4)
        overlay = np.full(act.shape, SENTINEL, np.float32, order="F")
        filled = np.zeros(act.shape, np.int32)
        for rank in range(4):
            r0, r1, c0, c1 = tiles.tile_rect(rank, g.mesh.nrow, g.mesh.ncol, pr, pc)
            s = _plan(g, _structure(name, g), tile=(r0, r1, c0, c1))
            ci = np.full(act.shape, SENTINEL, np.float32, order="F")
            s.adjust_interception(day, ci)
            s.close()
            own = np.zeros(act.shape, bool)
            own[r0:r1, c0:c1] = True
            wrote = _bits(ci) != _bits(np.full(act.shape, SENTINEL, np.float32))
            print(f"{name} tile {rank} rows [{r0}, {r1}) cols [{c0}, {c1}): wrote {int(wrote.sum())} cells, owns {int((own & act).sum())} active", flush=True)
            assert np.array_equal(wrote, own & act)
            overlay[wrote] = ci[wrote]
            filled += wrote
        assert np.array_equal(filled == 1, act)
        _check_plane(f"{name} [2 x 2 tiles overlaid]", overlay, ci_ref, act)


def step_refusals():
    """gr-a: E_UNSUPPORTED; no forcing: E_STATE; a malformed day_index handed straight to the C call: E_ARG; the plane untouched"""
    import ctypes as C
    import smash_amd
    from smash_amd import _lib
    g, day, nday, _ = iu.load("gr_b_16x16x96_nse_gaps")
    L = _lib.lib()
    day32 = np.ascontiguousarray(day, np.int32)
    ci = np.full((g.mesh.nrow, g.mesh.ncol), SENTINEL, np.float32, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def rc_of(s, nd, d, plane):
        rc = L.smashx_adjust_interception(s._h, nd, p(d) if d is not None else None, p(plane) if plane is not None else None)
        print("   rc", rc, L.smashx_last_error().decode() if rc else "", flush=True)
        return rc
    for st in ("gr-a", "gr-d", "vic-a"):
        s = _plan(g, st)
        assert rc_of(s, nday, day32, ci) == _lib.E_UNSUPPORTED, st
        with np.testing.assert_raises(smash_amd.SmashxError):
            s.adjust_interception(day)
        s.close()
    s = _plan(g, "gr-b", forcing=False)
    assert rc_of(s, nday, day32, ci) == _lib.E_STATE
    try:
        s.adjust_interception(day, ci)
        raise AssertionError("no error without forcing")
    except smash_amd.SmashxError as e:
        assert e.code == _lib.E_STATE
    s.close()
    s = _plan(g, "gr-b")
    assert rc_of(s, nday, None, ci) == _lib.E_ARG
    assert rc_of(s, nday, day32, None) == _lib.E_ARG
    assert rc_of(s, nday + 1, day32, ci) == _lib.E_ARG
    assert rc_of(s, nday - 1, day32, ci) == _lib.E_ARG
    for edit in (lambda d: d.__setitem__(0, 2), lambda d: d.__setitem__(slice(50, None), d[50:] + 2), lambda d: d.__setitem__(40, 1)):
        d = day32.copy(); edit(d)
        assert rc_of(s, int(d[-1]), d, ci) == _lib.E_ARG
    assert np.all(ci == SENTINEL)
    assert rc_of(s, nday, day32, ci) == 0 and not np.all(ci == SENTINEL)
    s.close()


def step_forward():
    """the drop-in writes parameters.ci, and a forward run with the adjusted plane equals a forward run with the fixture's plane"""
    import smash_amd
    from test_gpu_parity import _types
    for name in ("gr_b_16x16x96_nse_gaps", "gr_c_32x32x240_d8_ragged"):
        g, day, nday, ci_ref = iu.load(name)
        act = np.asarray(g.mesh.active_cell) == 1
        res = []
        for adjusted in (False, True):
            setup, mesh, inp, par, sta, out = _types(g)
            before = par.ci.copy()
            if adjusted:
                ret = smash_amd.adjust_interception_store(setup, mesh, inp, par, nday, day)
                assert ret is par.ci
                assert np.array_equal(_bits(par.ci[~act]), _bits(before[~act]))
            else:
                par.ci = np.asfortranarray(np.where(act, ci_ref, before).astype(np.float32))
            plane = par.ci.copy()
            smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], out, np.float32(0))
            res.append((plane, out.qsim.copy(), out.cost))
        ndiff = int(np.sum(_bits(res[0][1]) != _bits(res[1][1])))
        print(f"{name}: ci planes equal {np.array_equal(_bits(res[0][0]), _bits(res[1][0]))}, qsim values that differ {ndiff} of {res[0][1].size}, "
              f"cost {res[0][2]!r} / {res[1][2]!r}; moved from the fixture's own ci on {int(np.sum(res[1][0][act] != g.params['ci'][act]))} cells", flush=True)
        assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and ndiff == 0 and res[0][2] == res[1][2]
        assert np.any(res[1][0][act] != g.params["ci"][act])       # the run does depend on the plane: it is not the one the fixture carried


def step_at_size(n=1024, nt=8760, nsample=4096):
    """n^2 cells x nt steps, gr-b, compact forcing built on the device block by block as bench.py builds it; the columns of nsample
    randomly drawn active cells are gathered to the host from the very blocks handed to the library and put through the numpy
    restatement"""
    import torch
    import smash_amd
    import bench
    from smash_amd import synth
    from smash_amd.solver import Solver
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    t_all = time.perf_counter()
    m = synth.make_mesh(n, n, ng=1)
    setup = smash_amd.SetupDT(0, 0, structure="gr-b", dt=3600.0, ntime_step=nt)
    mesh = smash_amd.MeshDT(setup, n, n, 0)
    mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.dx, m.flwdir, m.flwacc, m.path, m.active_cell
    mesh.gauge_pos, mesh.area = np.zeros((0, 2), np.int32, order="F"), np.zeros(0, np.float32)
    sol = Solver(setup, mesh)
    daily, w = synth._pet_tables()
    sol.set_forcing_layout(compact=True, prcp_factor=0.1, pet_ratio=w, pet_hour0=0)
    rows, cols = sol.cell_order()
    rng = np.random.default_rng(20141015)
    pick = np.sort(rng.choice(sol.ncells, size=min(nsample, sol.ncells), replace=False))
    d_pick = torch.from_numpy(pick.astype(np.int64)).to(dev)
    d_rows = torch.from_numpy(rows.astype(np.int64)).to(dev)
    d_cols = torch.from_numpy(cols.astype(np.int64)).to(dev)
    tb = max(24, (1 << 26) // max(sol.ncells, 1) // 24 * 24)
    hp, he = [], []
    for t0 in range(0, nt, tb):
        t1 = min(nt, t0 + tb)
        prcp, pet = bench.forcing_block(d_rows, d_cols, t0, t1, dev)
        torch.cuda.synchronize()
        sol.set_forcing_device_block(t0, t1, prcp.data_ptr(), pet.data_ptr())
        hp.append(prcp.index_select(1, d_pick).cpu().numpy()); he.append(pet.index_select(1, d_pick).cpu().numpy())
        del prcp, pet
    del d_rows, d_cols
    torch.cuda.empty_cache()
    info = sol.forcing_info()
    assert info["layout"].startswith("compact"), info
    print(f"at size: {sol.ncells} cells x {nt} steps, forcing {info['layout'].split(':')[0]} ({info['resident_bytes_per_cellstep']} B per cell-step), "
          f"set-up {time.perf_counter() - t_all:.1f} s", flush=True)
    # pet_hour0 = 0: step 0 is hour 0 of day 1 (a run that starts at 23:00 the evening before)
    day = smash_amd.day_index("2014-09-14 23:00", np.datetime64("2014-09-14T23:00") + np.timedelta64(3600 * nt, "s"), 3600)
    assert np.array_equal(day, 1 + np.arange(nt) // 24)
    ci = np.full((n, n), SENTINEL, np.float32, order="F")
    t0 = time.perf_counter()
    sol.adjust_interception(day, ci)
    wall = time.perf_counter() - t0
    print(f"at size: smashx_adjust_interception took {wall:.3f} s wall = {sol.ncells * nt / wall:.3e} 49-candidate cell-steps/s", flush=True)
    sol.close()
    t0 = time.perf_counter()
    mine, diff = iu.adjust(np.concatenate(hp, axis=0).T, np.concatenate(he, axis=0).T, day)
    got = ci[rows[pick], cols[pick]]
    nbad = int(np.sum(_bits(got) != _bits(mine)))
    act = np.asarray(m.active_cell) == 1
    print(f"at size: {pick.size} sampled cells, {np.unique(mine).size} distinct ci in the sample, {iu.exact_ties(diff)} with an exact tie of the two "
          f"best candidates, {nbad} differ from the numpy restatement ({time.perf_counter() - t0:.1f} s of numpy); "
          f"{np.unique(ci[act]).size} distinct ci over the grid", flush=True)
    assert nbad == 0
    assert np.all(np.isin(_bits(ci[act]), _bits(iu.candidates()))) and np.all(ci[~act] == SENTINEL)


STEPS = {"fixtures": step_fixtures, "cance_compact": step_cance_compact, "tiles": step_tiles, "refusals": step_refusals,
         "forward": step_forward, "at_size": step_at_size}

if __name__ == "__main__":
    import torch  # noqa: F401  (its HIP runtime must initialise before libsmashx's: tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    STEPS[sys.argv[1]](*[int(v) for v in sys.argv[2:]])
    print("OK", sys.argv[1], "exact-libm build" if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0") else "default build", flush=True)
