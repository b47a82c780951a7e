"""GPU steps of tests/test_gpu_prcp_indices.py, one per child process (python prcp_indices_worker.py <step>), so that every step has a
time limit of its own and the library build (SMASHX_EXACT_LIBM) is chosen per step.  Every comparison is exact equality of fp32 bit
patterns with NaN = NaN (prcp_indices_util.same_bits) over the whole (4, ng, nt) array, so the entries a call must leave alone are
compared with the sentinel they were given; each figure is printed before it is asserted."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import mean_forcing_util as mu                                             # noqa: E402
import prcp_indices_util as pu                                             # noqa: E402
from mean_forcing_worker import _pieces_case, _plan, _synth_layout         # noqa: E402

F = np.float32


def _check(tag, got, want):
    bad = pu.count_differing(got, want)
    left = np.all(got == pu.SENTINEL, axis=0)
    same_left = bool(np.array_equal(left, np.all(want == pu.SENTINEL, axis=0)))
    print(f"{tag}: {got.shape[1]} gauges x {got.shape[2]} steps, {int((~left).sum())} pairs written, {int(left.sum())} untouched (the same set: {same_left}), "
          f"NaN entries {int(np.isnan(got).sum())}, {bad} entries differ from the reference", flush=True)
    assert bad == 0 and same_left, tag


def step_fixtures():
    """every fixture in dense, sparse and compact residency against the reference's array"""
    for name in sorted(pu.CASES):
        g, prcp, flwdst, ref = pu.load(name)
        layouts = [("dense", dict()), ("sparse", dict(sparse=True))]
        if "cance" in name:          # Cance's rain went through float64: the plan stays in fp32 rows
            layouts.append(("compact-requested", dict(layout=dict(compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1))))
        else:
            layouts.append(("compact", dict(layout=_synth_layout())))
        for tag, kw in layouts:
            s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, **kw)
            info = s.forcing_info()["layout"]
            if tag == "compact":
                assert info.startswith("compact"), info
            out = pu.sentinels(g.mesh.ng, g.nt)
            assert s.prcp_indices(flwdst, out) is out
            _check(f"{name} [{tag}: {info.split(':')[0]}]", out, ref)
            s.close()


def step_pieces():
    """96 x 96 x 200: the lists cut into pieces of 4096 entries (5 launches for the outlet's catchment + bins) against the restatement
    and the default piece"""
    m, nt, prcp, pet = _pieces_case()
    from smash_amd import synth
    flwdst = synth.flow_distance(m.flwdir, m.active_cell, m.dx)
    tabs = pu.gauge_tables(m.flwdir, m.gauge_pos, flwdst)
    pad = lambda n: -(-n // 64) * 64      # noqa: E731
    entries = [pad(T["rows"].size) + sum(pad(br.size) for br, _ in T["bins"]) for T in tabs]
    piece = 4096
    assert tabs[0]["rows"].size == 96 * 96 and -(-max(entries) // piece) == 5, entries
    assert int((prcp < 0).sum()) > 0 and nt % 64 != 0
    want = pu.sentinels(m.ng, nt)
    written = pu.prcp_indices(m.flwdir, m.gauge_pos, flwdst, prcp, want)
    assert 64 <= int(written.sum()) < written.size - 8
    for tag, lay in (("compact", _synth_layout()), ("fp32 rows", None)):
        res = {}
        for forced in (False, True):
            if forced:
                os.environ["SMASHX_PI_PIECE"] = str(piece)
            else:
                os.environ.pop("SMASHX_PI_PIECE", None)
            s = _plan(m, nt, prcp, pet, layout=lay)
            info = s.forcing_info()["layout"]
            assert info.startswith(tag), info
            out = pu.sentinels(m.ng, nt)
            s.prcp_indices(flwdst, out)
            s.close()
            _check(f"96 x 96 x 200 [{tag}], list entries {entries}, piece {piece if forced else 'default'} vs the numpy restatement", out, want)
            res[forced] = out
        os.environ.pop("SMASHX_PI_PIECE", None)
        assert pu.same_bits(res[False], res[True])


def step_block_pieces():
    """a launch boundary on every block boundary (SMASHX_PI_PIECE = 64), so that every section boundary and every bin-completing block
    falls on one: gr_c_32x32x240_d8_ragged in compact and in fp32 rows against the fixture, the untouched set included, and against
    the default piece.  The library reports its launches on stderr (SMASHX_VERBOSE), which the test compares with the blocks"""
    os.environ["SMASHX_VERBOSE"] = "1"
    name = "gr_c_32x32x240_d8_ragged"
    g, prcp, flwdst, ref = pu.load(name)
    for tag, lay in (("compact", _synth_layout()), ("fp32 rows", None)):
        res = {}
        for forced in (False, True):
            if forced:
                os.environ["SMASHX_PI_PIECE"] = "64"
            else:
                os.environ.pop("SMASHX_PI_PIECE", None)
            s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, layout=lay)
            info = s.forcing_info()["layout"]
            assert info.startswith(tag), info
            out = pu.sentinels(g.mesh.ng, g.nt)
            s.prcp_indices(flwdst, out)
            s.close()
            _check(f"{name} [{tag}], piece {64 if forced else 'default'}", out, ref)
            res[forced] = out
        os.environ.pop("SMASHX_PI_PIECE", None)
        assert pu.same_bits(res[False], res[True])


def step_second_plane():
    """a second call with another flwdst gives that plane's result, the first plane again the first result; smashx_mean_forcing
    before, between and after stays bit-equal to its fixture"""
    name = "gr_c_32x32x240_d8_ragged"
    g, prcp, flwdst, ref = pu.load(name)
    _, _, _, mp_ref, me_ref = mu.load(name)
    other = np.asfortranarray(np.where(flwdst < 0, flwdst, np.sqrt(flwdst) * F(3.0)).astype(F))     # another metric on the same tree
    want = pu.sentinels(g.mesh.ng, g.nt)
    pu.prcp_indices(g.mesh.flwdir, g.mesh.gauge_pos, other, prcp, want)
    assert pu.count_differing(want, ref) >= 64
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, layout=_synth_layout())

    def means(tag):
        mp, me = s.mean_forcing()
        print(f"{name}: mean_forcing {tag}: {mu.count_differing(mp, mp_ref)} + {mu.count_differing(me, me_ref)} differ from its fixture", flush=True)
        assert mu.same_bits(mp, mp_ref) and mu.same_bits(me, me_ref)
    means("before")
    for tag, plane, w in (("first plane", flwdst, ref), ("second plane", other, want), ("first plane again", flwdst, ref)):
        out = pu.sentinels(g.mesh.ng, g.nt)
        s.prcp_indices(plane, out)
        _check(f"{name}: {tag}", out, w)
        means("after the " + tag)
    s.close()
    # the other order: indices first, on a plan that has not built its catchment lists yet
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt)
    out = pu.sentinels(g.mesh.ng, g.nt)
    s.prcp_indices(flwdst, out)
    _check(f"{name}: indices before any mean_forcing call", out, ref)
    means("after the indices")
    s.close()


def step_refusals():
    """no forcing: E_STATE; a NULL argument: E_ARG; a tiled plan, a one-cell catchment, a (row, row) cell that is inactive or outside
    the grid: E_UNSUPPORTED; ng = 0: OK and nothing written.  Every refusal is an argument check that returns a code; the buffer
    keeps the sentinel throughout"""
    import smash_amd
    from smash_amd import _lib, synth, tiles
    g, prcp, flwdst, ref = pu.load("gr_b_16x16x96_nse_gaps")
    L = _lib.lib()
    out = pu.sentinels(g.mesh.ng, g.nt)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731

    def rc_of(handle, a, b):
        rc = L.smashx_prcp_indices(handle, p(a), p(b))
        print("   rc", rc, L.smashx_last_error().decode() if rc else "", flush=True)
        return rc
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, forcing=False)
    assert rc_of(s._h, flwdst, out) == _lib.E_STATE
    try:
        s.prcp_indices(flwdst, out)
        raise AssertionError("no error without forcing")
    except smash_amd.SmashxError as e:
        assert e.code == _lib.E_STATE
    s.close()
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt)
    assert rc_of(s._h, None, out) == _lib.E_ARG
    assert rc_of(s._h, flwdst, None) == _lib.E_ARG
    assert rc_of(None, flwdst, out) == _lib.E_ARG
    s.close()
    pr, pc = tiles.tile_grid(4)
    for rank in range(4):
        s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, tile=tiles.tile_rect(rank, g.mesh.nrow, g.mesh.ncol, pr, pc), gauges=False)
        assert rc_of(s._h, flwdst, out) == _lib.E_UNSUPPORTED, rank
        s.close()
    assert np.all(out == pu.SENTINEL)

    def regauged(m, pos):
        return synth.Mesh(m.nrow, m.ncol, m.dx, m.flwdir, m.flwacc, m.path, m.active_cell, np.array([pos], np.int32),
                          np.array([float(m.flwacc[pos]) * m.dx * m.dx], np.float32))

    def refused(m, what):
        dst = synth.flow_distance(m.flwdir, m.active_cell, m.dx)
        hp, he = synth.dense_forcing(m, 48)
        s = _plan(m, 48, hp, he)
        a = pu.sentinels(1, 48)
        print(what, flush=True)
        assert rc_of(s._h, dst, a) == _lib.E_UNSUPPORTED
        assert rc_of(s._h, dst, a) == _lib.E_UNSUPPORTED
        assert np.all(a == pu.SENTINEL)
        s.close()
    # a headwater gauge: its catchment is itself
    m = synth.make_mesh(16, 16, ng=1)
    assert int(mu.upstream(m.flwdir, 0, 0).sum()) == 1
    refused(regauged(m, (0, 0)), "a one-cell catchment")
    # the north-west block is inactive; a gauge in row 2 east of it: the cell (2, 2) the reference reads is inactive
    m = synth.make_mesh(16, 16, ng=1, mask_corner=True)
    col = next(c for c in range(6, 16) if int(mu.upstream(m.flwdir, 2, c).sum()) >= 2)
    assert m.active_cell[2, 2] == 0 and m.active_cell[2, col] == 1 and np.all(m.active_cell[mu.upstream(m.flwdir, 2, col)] == 1)
    refused(regauged(m, (2, col)), f"gauge (2, {col}): the cell (2, 2) is inactive")
    # more rows than columns: the outlet's row is no column of the grid
    m = synth.make_mesh(24, 8, ng=1)
    assert tuple(m.gauge_pos[0]) == (23, 7)
    refused(m, "gauge (23, 7) on a 24 x 8 grid: the cell (23, 23) is outside the grid")
    # no gauges: OK, nothing written
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt, gauges=False)
    assert rc_of(s._h, flwdst, out) == 0
    assert np.all(out == pu.SENTINEL)
    s.close()
    # and the call does work on this mesh
    s = _plan(g.mesh, g.nt, prcp, g.pet, dt=g.dt)
    assert rc_of(s._h, flwdst, out) == 0
    _check("gr_b_16x16x96_nse_gaps after the refusals", out, ref)
    s.close()


def step_python():
    """smash_amd.compute_prcp_indices updates the caller's array in place; smash_amd.prcp_indices returns the four (ng, nt) arrays with
    NaN where the reference's wrapper puts it"""
    import smash_amd
    from test_gpu_parity import _types
    for name in ("gr_b_16x16x96_nse_gaps", "gr_c_32x32x240_d8_ragged"):
        g, prcp, flwdst, ref = pu.load(name)
        setup, mesh, inp, par, sta, _ = _types(g)
        assert np.array_equal(mesh.flwdst.view(np.uint32), flwdst.view(np.uint32))
        out = pu.sentinels(g.mesh.ng, g.nt)
        assert smash_amd.compute_prcp_indices(setup, mesh, inp, out) is out
        _check(f"{name}: compute_prcp_indices(setup, mesh, input_data, prcp_indices)", out, ref)
        res = smash_amd.prcp_indices(setup, mesh, inp)
        assert list(res) == ["std", "d1", "d2", "vg"]
        written = ~np.all(ref == pu.SENTINEL, axis=0)
        for i, k in enumerate(res):
            a = res[k]
            want = np.where(written, np.where(ref[i] < 0, F(np.nan), ref[i]), F(np.nan)).astype(F)
            print(f"{name}: prcp_indices()[{k!r}]: {pu.count_differing(a, want)} differ, {int(np.isnan(a).sum())} NaN", flush=True)
            assert a.shape == (g.mesh.ng, g.nt) and a.dtype == F and pu.same_bits(a, want)


STEPS = {"fixtures": step_fixtures, "pieces": step_pieces, "block_pieces": step_block_pieces, "second_plane": step_second_plane, "refusals": step_refusals, "python": step_python}

if __name__ == "__main__":
    import torch  # noqa: F401  (its HIP runtime must initialise before libsmashx's: tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    STEPS[sys.argv[1]]()
    print("OK", sys.argv[1], "exact-libm build" if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0") else "default build", flush=True)
