"""GPU steps of tests/test_gpu_mean_forcing.py, one per child process (python mean_forcing_worker.py <step>), so that every step has a
time limit of its own and the library build (SMASHX_EXACT_LIBM) is chosen per step.  Every comparison is exact equality of fp32 bit
patterns with NaN = NaN (mean_forcing_util.same_bits); each figure is printed before it is asserted."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import golden_util as gu             # noqa: E402,F401
import mean_forcing_util as mu       # noqa: E402

SENTINEL = np.float32(-7.0)
F = np.float32


def _sparse_order(m):
    """(rows, cols) of the active cells along mesh%path: the numbering of the (nac, nt) sparse vectors (mw_sparse_storage.f90:12-49)"""
    path, act = np.asarray(m.path), np.asarray(m.active_cell)
    keep = (path[0] >= 0) & (path[1] >= 0)
    keep[keep] &= act[path[0][keep], path[1][keep]] == 1
    return path[0][keep], path[1][keep]


def _plan(m, nt, prcp, pet, dt=3600.0, sparse=False, layout=None, tile=None, forcing=True, gauges=True):
    """a gr-b plan on mesh m with its gauges (the routine reads the forcing, the flow directions and the gauge positions)"""
    import smash_amd
    from smash_amd.solver import Solver
    ng = m.ng if gauges else 0
    setup = smash_amd.SetupDT(0, ng, structure="gr-b", dt=dt, ntime_step=nt, sparse_storage=sparse)
    mesh = smash_amd.MeshDT(setup, m.nrow, m.ncol, ng)
    mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.dx, m.flwdir, m.flwacc, m.path, m.active_cell
    if gauges:
        mesh.gauge_pos, mesh.area = m.gauge_pos, m.area
    else:
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


def _sentinels(ng, nt):
    return np.full((ng, nt), SENTINEL, F, order="F"), np.full((ng, nt), SENTINEL, F, order="F")


def _check(tag, got, want):
    bad = [mu.count_differing(a, b) for a, b in zip(got, want)]
    left = [int(np.sum(a == SENTINEL)) for a in got]
    print(f"{tag}: {got[0].shape[0]} gauges x {got[0].shape[1]} steps, NaN steps {int(np.isnan(got[0]).sum())} + {int(np.isnan(got[1]).sum())}, "
          f"{bad[0]} + {bad[1]} differ from the reference, {left[0]} + {left[1]} kept the sentinel", flush=True)
    assert bad == [0, 0] and left == [0, 0], tag


def _synth_layout():
    from smash_amd import synth
    return dict(compact=True, prcp_factor=0.1, pet_ratio=synth._pet_tables()[1], pet_hour0=0)


def step_fixtures():
    """every fixture in dense, sparse and compact residency against the reference's arrays"""
    for name in sorted(mu.CASES):
        g, prcp, pet, mp_ref, me_ref = mu.load(name)
        layouts = [("dense", dict()), ("sparse", dict(sparse=True))]
        if "cance" in name:
            layouts.append(("compact-requested", dict(layout=dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1))))
        elif name in mu.BLANK:        # PET blanked at one hour of a day is not daily x ratio: the plan stays in fp32 rows
            layouts.append(("compact-requested", dict(layout=_synth_layout())))
        else:
            layouts.append(("compact", dict(layout=_synth_layout())))
        for tag, kw in layouts:
            s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, **kw)
            info = s.forcing_info()["layout"]
            if tag == "compact":
                assert info.startswith("compact"), info
            mp, me = _sentinels(g.mesh.ng, g.nt)
            out = s.mean_forcing(mp, me)
            assert out[0] is mp and out[1] is me
            _check(f"{name} [{tag}: {info.split(':')[0]}]", (mp, me), (mp_ref, me_ref))
            s.close()


def step_cance_compact():
    """Cance with both fields put on the fp32 reader's form (real(k) * 0.1, daily * ratio(hour) as float32 products: what the
    reference's reader produces), which loads into the compact layout; the yardstick on this forcing is the numpy restatement, and the
    fp32-rows plan on the same forcing must agree as well"""
    from smash_amd.solver import RATIO_PET_HOURLY as R
    g, gp, ge, _, _ = mu.load("gr_a_cance_28x28x1440")
    prcp = np.asfortranarray(np.where(gp < 0, gp, np.rint(gp / F(0.1)).astype(F) * F(0.1)).astype(F))
    pet = ge.copy(order="F")
    for d in range((g.nt + 1 + 23) // 24):
        ts = list(range(max(0, d * 24 - 1), min(g.nt, (d + 1) * 24 - 1)))
        tb = max(ts, key=lambda t: R[(t + 1) % 24])
        daily = (pet[:, :, tb] / R[(tb + 1) % 24]).astype(F) if R[(tb + 1) % 24] > 0 else np.zeros(pet.shape[:2], F)
        for t in ts:
            pet[:, :, t] = daily * R[(t + 1) % 24]
    want = mu.mean_forcing(g.mesh.flwdir, g.mesh.gauge_pos, prcp, pet)
    for tag, lay in (("compact", dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1)), ("fp32 rows", None)):
        s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, layout=lay)
        info = s.forcing_info()["layout"]
        assert info.startswith(tag), info
        mp, me = _sentinels(g.mesh.ng, g.nt)
        s.mean_forcing(mp, me)
        _check(f"cance on the reader's form [{tag}] vs the numpy restatement", (mp, me), want)
        s.close()


def _pieces_case():
    """96 x 96 cells x 200 steps (not a multiple of 64), an outlet gauge whose list is the whole grid (9216 cells) and two nested ones;
    rain gaps on 2 % of the cell-steps, PET gap days on a seventh of the cells"""
    from smash_amd import synth
    m = synth.make_mesh(96, 96, ng=3)
    nt = 200
    prcp, pet = synth.dense_forcing(m, nt, gap_per_million=20000)
    r, c = np.meshgrid(np.arange(96), np.arange(96), indexing="ij")
    holes = (r + 2 * c) % 7 == 0
    for day in (1, 4):
        pet[holes, day * 24:(day + 1) * 24] = F(-99.0)
    return m, nt, prcp, pet


def step_pieces():
    """the list cut into pieces of 2048 entries (5 launches for the 9216-cell list) against the restatement and the default piece"""
    m, nt, prcp, pet = _pieces_case()
    masks = mu.gauge_masks(m)
    sizes = [int(k.sum()) for k in masks]
    assert sizes[0] == 96 * 96 and all(0 < k < sizes[0] for k in sizes[1:]), sizes
    assert int((prcp < 0).sum()) > 0 and int((pet < 0).sum()) > 0 and nt % 64 != 0
    want = mu.mean_forcing(m.flwdir, m.gauge_pos, prcp, pet)
    piece = 2048
    assert -(-sizes[0] // piece) >= 5
    for tag, lay in (("compact", _synth_layout()), ("fp32 rows", None)):
        res = {}
        for forced in (False, True):
            if forced:
                os.environ["SMASHX_MF_PIECE"] = str(piece)
            else:
                os.environ.pop("SMASHX_MF_PIECE", None)
            s = _plan(m, nt, prcp, pet, layout=lay)
            info = s.forcing_info()["layout"]
            assert info.startswith(tag), info
            mp, me = _sentinels(m.ng, nt)
            s.mean_forcing(mp, me)
            s.close()
            _check(f"96 x 96 x 200 [{tag}], catchments {sizes}, piece {piece if forced else 'default'} vs the numpy restatement", (mp, me), want)
            res[forced] = (mp, me)
        os.environ.pop("SMASHX_MF_PIECE", None)
        assert mu.same_bits(res[False][0], res[True][0]) and mu.same_bits(res[False][1], res[True][1])


def _forced_and_default(tag, m, nt, prcp, pet, lay, want, dt=3600.0):
    """the default piece and SMASHX_MF_PIECE = 64 (one block per launch) against want and against each other"""
    res = {}
    for forced in (False, True):
        if forced:
            os.environ["SMASHX_MF_PIECE"] = "64"
        else:
            os.environ.pop("SMASHX_MF_PIECE", None)
        s = _plan(m, nt, prcp, pet, dt=dt, layout=lay)
        mp, me = _sentinels(m.ng, nt)
        s.mean_forcing(mp, me)
        info = s.forcing_info()["layout"]
        s.close()
        _check(f"{tag} [{info.split(':')[0]}], piece {64 if forced else 'default'}", (mp, me), want)
        res[forced] = (mp, me)
    os.environ.pop("SMASHX_MF_PIECE", None)
    assert mu.same_bits(res[False][0], res[True][0]) and mu.same_bits(res[False][1], res[True][1])
    return info


def step_block_pieces():
    """a launch boundary on every block boundary (SMASHX_MF_PIECE = 64): gr_c_32x32x240_d8_ragged, whose largest list is 561 cells = 9
    blocks, the last one partly padding, over 240 steps (not a multiple of 64), against the fixture and the default piece; and an 8 x 8
    mesh whose outlet catchment is exactly 64 cells, one full block without a padding entry, against the numpy restatement.  Compact
    and fp32 rows; the library reports its launches on stderr (SMASHX_VERBOSE), which the test counts"""
    from smash_amd import synth
    os.environ["SMASHX_VERBOSE"] = "1"
    name = "gr_c_32x32x240_d8_ragged"
    g, prcp, pet, mp_ref, me_ref = mu.load(name)
    sizes = [int(k.sum()) for k in mu.gauge_masks(g.mesh)]
    assert max(sizes) == 561 and -(-max(sizes) // 64) == 9 and max(sizes) % 64 != 0 and g.nt == 240, (sizes, g.nt)
    m = synth.make_mesh(8, 8, ng=1)
    nt = 100
    assert int(mu.gauge_masks(m)[0].sum()) == 64 and nt % 64 != 0
    sp, se = synth.dense_forcing(m, nt, gap_per_million=20000)
    assert int((sp < 0).sum()) > 0
    want = mu.mean_forcing(m.flwdir, m.gauge_pos, sp, se)
    for tag, lay in (("compact", _synth_layout()), ("fp32 rows", None)):
        info = _forced_and_default(f"{name}, catchments {sizes}", g.mesh, g.nt, prcp, pet, lay, (mp_ref, me_ref), dt=g.dt)
        assert info.startswith(tag), info
        info = _forced_and_default("8 x 8 x 100, a catchment of 64 cells vs the numpy restatement", m, nt, sp, se, lay, want)
        assert info.startswith(tag), info


def step_one_output():
    """mean_pet = NULL and mean_prcp = NULL: the half that is asked for equals the full call's and is fully overwritten"""
    for name, lay in (("gr_b_16x16x96_nse_gaps__blank", _synth_layout()), ("gr_c_32x32x240_d8_ragged", None)):
        g, prcp, pet, mp_ref, me_ref = mu.load(name)
        s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, layout=lay)
        full = _sentinels(g.mesh.ng, g.nt)
        s.mean_forcing(*full)
        _check(f"{name}: both outputs", full, (mp_ref, me_ref))
        only_p, _ = _sentinels(g.mesh.ng, g.nt)
        out = s.mean_forcing(only_p, None, pet=False)
        assert out[0] is only_p and out[1] is None
        only_e, _ = _sentinels(g.mesh.ng, g.nt)
        out = s.mean_forcing(None, only_e, prcp=False)
        assert out[0] is None and out[1] is only_e
        s.close()
        print(f"{name}: prcp alone differs on {mu.count_differing(only_p, full[0])}, pet alone on {mu.count_differing(only_e, full[1])}, "
              f"sentinels left {int(np.sum(only_p == SENTINEL))} + {int(np.sum(only_e == SENTINEL))}", flush=True)
        assert mu.same_bits(only_p, full[0]) and mu.same_bits(only_e, full[1])
        assert not np.any(only_p == SENTINEL) and not np.any(only_e == SENTINEL)


def step_refusals():
    """no forcing: E_STATE; both outputs NULL or plan NULL: E_ARG; a tiled plan and a catchment with an inactive cell: E_UNSUPPORTED;
    ng = 0: OK and nothing written.  The buffers keep the sentinel throughout"""
    import smash_amd
    from smash_amd import _lib, synth, tiles
    g, prcp, pet, mp_ref, me_ref = mu.load("gr_b_16x16x96_nse_gaps")
    L = _lib.lib()
    mp, me = _sentinels(g.mesh.ng, g.nt)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731

    def rc_of(handle, a, b):
        rc = L.smashx_mean_forcing(handle, p(a), p(b))
        print("   rc", rc, L.smashx_last_error().decode() if rc else "", flush=True)
        return rc
    s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, forcing=False)
    assert rc_of(s._h, mp, me) == _lib.E_STATE
    try:
        s.mean_forcing(mp, me)
        raise AssertionError("no error without forcing")
    except smash_amd.SmashxError as e:
        assert e.code == _lib.E_STATE
    s.close()
    s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt)
    assert rc_of(s._h, None, None) == _lib.E_ARG
    assert rc_of(None, mp, me) == _lib.E_ARG
    assert np.all(mp == SENTINEL) and np.all(me == SENTINEL)
    s.close()
    # a 2 x 2 tiling: every part refuses
    pr, pc = tiles.tile_grid(4)
    for rank in range(4):
        s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, tile=tiles.tile_rect(rank, g.mesh.nrow, g.mesh.ncol, pr, pc), gauges=False)
        assert rc_of(s._h, mp, me) == _lib.E_UNSUPPORTED, rank
        s.close()
    # a gauge that drains an inactive cell: a headwater cell of the outlet's catchment is switched off, its flow direction stays
    m = synth.make_mesh(16, 16, ng=1)
    act = np.array(m.active_cell, order="F")
    assert m.flwdir[0, 0] in (3, 4, 5) and tuple(m.gauge_pos[0]) != (0, 0)
    act[0, 0] = 0
    flwacc = synth.flow_accumulation(m.flwdir, act)
    hole = synth.Mesh(16, 16, m.dx, m.flwdir, flwacc, synth.make_path(np.where(act == 1, flwacc, -99)), act, m.gauge_pos, m.area)
    assert mu.upstream(hole.flwdir, *hole.gauge_pos[0])[0, 0]
    hp, he = synth.dense_forcing(hole, 48)
    s = _plan(hole, 48, hp, he)
    a, b = _sentinels(1, 48)
    assert rc_of(s._h, a, b) == _lib.E_UNSUPPORTED
    assert rc_of(s._h, a, b) == _lib.E_UNSUPPORTED          # the refusal is remembered with the plan
    assert np.all(a == SENTINEL) and np.all(b == SENTINEL)
    s.close()
    # no gauges: OK, nothing written (the buffers handed over belong to nobody)
    s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt, gauges=False)
    assert rc_of(s._h, mp, me) == 0
    assert np.all(mp == SENTINEL) and np.all(me == SENTINEL)
    s.close()
    # and the call does work on this mesh
    s = _plan(g.mesh, g.nt, prcp, pet, dt=g.dt)
    assert rc_of(s._h, mp, me) == 0
    _check("gr_b_16x16x96_nse_gaps after the refusals", (mp, me), (mp_ref, me_ref))
    s.close()


def step_python():
    """smash_amd.compute_mean_forcing fills input_data.mean_prcp / mean_pet with the fixture's arrays"""
    import smash_amd
    from test_gpu_parity import _types
    for name in ("gr_b_16x16x96_nse_gaps", "gr_c_32x32x240_d8_ragged"):
        g, prcp, pet, mp_ref, me_ref = mu.load(name)
        setup, mesh, inp, par, sta, out = _types(g)
        assert inp.mean_prcp.shape == (g.mesh.ng, g.nt) and np.all(inp.mean_prcp == F(-99.0)) and np.all(inp.mean_pet == F(-99.0))
        held = (inp.mean_prcp, inp.mean_pet)
        ret = smash_amd.compute_mean_forcing(setup, mesh, inp)
        assert ret[0] is inp.mean_prcp and ret[1] is inp.mean_pet and inp.mean_prcp is held[0] and inp.mean_pet is held[1]
        assert inp.mean_prcp.flags.f_contiguous and inp.mean_prcp.dtype == F
        _check(f"{name}: compute_mean_forcing(setup, mesh, input_data)", (inp.mean_prcp, inp.mean_pet), (mp_ref, me_ref))


STEPS = {"fixtures": step_fixtures, "cance_compact": step_cance_compact, "pieces": step_pieces, "block_pieces": step_block_pieces, "one_output": step_one_output,
         "refusals": step_refusals, "python": step_python}

if __name__ == "__main__":
    import torch  # noqa: F401  (its HIP runtime must initialise before libsmashx's: tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    STEPS[sys.argv[1]]()
    print("OK", sys.argv[1], "exact-libm build" if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0") else "default build", flush=True)
