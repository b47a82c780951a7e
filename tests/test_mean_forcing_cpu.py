"""CPU: the catchment-mean forcing (compute_mean_forcing, mw_forcing_statistic.f90:18-75) -- the numpy restatement against the fixtures
recorded from the compiled reference (exact equality of fp32 bit patterns, NaN = NaN), what makes the fixtures worth recording, the
upstream masks inside the active cells on every golden case, every argument error of check_mean_forcing raised before anything reaches
a device, and the new entry point declared on both sides of the ABI.  Runs without a GPU."""
import glob
import os

import numpy as np
import pytest

import golden_util as gu
import mean_forcing_util as mu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32


# ---- the restatement is the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mu.CASES))
def test_numpy_restatement_equals_the_reference(name):
    g, prcp, pet, mp, me = mu.load(name)
    assert mp.shape == me.shape == (g.mesh.ng, g.nt) and mp.dtype == F and me.dtype == F
    mine = mu.mean_forcing(g.mesh.flwdir, g.mesh.gauge_pos, prcp, pet)
    assert mine[0].dtype == F and mine[1].dtype == F
    assert mu.same_bits(mine[0], mp) and mu.same_bits(mine[1], me)


def test_fixture_files_hold_the_means_and_the_variant_only():
    for name in mu.CASES:
        z = np.load(os.path.join(mu.DIR, name + ".npz"))
        assert sorted(z.files) == ["blank_pet", "blank_prcp", "case", "mean_pet", "mean_prcp"], name
        assert str(z["case"]) == mu.CASES[name]
        b = mu.BLANK.get(name, dict(prcp=(), pet=()))
        assert z["blank_prcp"].tolist() == list(b["prcp"]) and z["blank_pet"].tolist() == list(b["pet"])
    assert sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(mu.DIR, "*.npz"))) == sorted(mu.CASES)


@pytest.mark.parametrize("name", sorted(mu.CASES))
def test_fixture_tells_a_sequential_sum_from_a_reassociated_one(name):
    """on at least 8 (gauge, step) pairs the recorded mean differs from the one formed from the fp64 sum rounded once"""
    g, prcp, pet, mp, me = mu.load(name)
    wide = mu.fp64_means(g.mesh.flwdir, g.mesh.gauge_pos, prcp, pet)
    assert mu.count_differing(mp, wide[0]) + mu.count_differing(me, wide[1]) >= 8


def test_same_bits_takes_nan_for_nan_and_nothing_else():
    a = np.array([1.0, np.nan, 0.0], F)
    b = a.copy()
    b.view(np.uint32)[1] ^= 0x80000000                       # the other sign of NaN
    assert mu.same_bits(a, b) and mu.count_differing(a, b) == 0
    assert not mu.same_bits(a, np.array([1.0, np.nan, -0.0], F))
    assert not mu.same_bits(a, np.array([1.0, 2.0, 0.0], F)) and mu.count_differing(a, np.array([1.0, 2.0, 0.0], F)) == 1


def test_blanked_steps_and_only_they_are_nan():
    name = "gr_b_16x16x96_nse_gaps__blank"
    g, prcp, pet, mp, me = mu.load(name)
    b = mu.BLANK[name]
    want_p, want_e = np.zeros(mp.shape, bool), np.zeros(me.shape, bool)
    want_p[:, list(b["prcp"])] = True
    want_e[:, list(b["pet"])] = True
    assert len(b["prcp"]) == 2 and len(b["pet"]) == 1
    assert np.array_equal(np.isnan(mp), want_p) and np.array_equal(np.isnan(me), want_e)
    for other in set(mu.CASES) - {name}:
        _, _, _, op, oe = mu.load(other)
        assert not np.isnan(op).any() and not np.isnan(oe).any(), other


def test_gaps_case_is_partially_gapped_on_every_step():
    """0 < count < |catchment| of the outlet gauge's rain on every step: the mask matters everywhere and never empties the sum"""
    g, prcp, pet, mp, me = mu.load("gr_b_16x16x96_nse_gaps")
    _, _, cp, ce = mu.mean_forcing(g.mesh.flwdir, g.mesh.gauge_pos, prcp, pet, counts=True)
    sizes = [int(k.sum()) for k in mu.gauge_masks(g.mesh)]
    out = int(np.argmax(sizes))
    assert np.all(cp[out] > 0) and np.all(cp[out] < sizes[out])
    assert np.all(cp > 0) and np.all(ce > 0)


def test_catchment_sizes_of_the_cases():
    want = {"gr_a_cance_28x28x1440": [383, 108, 28], "gr_c_32x32x240_d8_ragged": 561, "gr_b_64x64x720_nse": 4096}
    for name, w in want.items():
        sizes = [int(k.sum()) for k in mu.gauge_masks(gu.load(name).mesh)]
        assert (sizes == w) if isinstance(w, list) else (max(sizes) == w and len(sizes) == 4), (name, sizes)


# ---- upstream() ---------------------------------------------------------------------------------------------------------------------
def _golden_cases():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(gu.GOLDEN_DIR, "*.npz")))


def test_upstream_masks_lie_inside_the_active_cells_on_every_golden_case():
    cases = _golden_cases()
    assert len(cases) == 18
    for case in cases:
        m = gu.load(case).mesh
        act = np.asarray(m.active_cell) == 1
        gp = np.asarray(m.gauge_pos).reshape(-1, 2)
        for k, (r, c) in zip(mu.gauge_masks(m), gp):
            assert k[r, c] and np.all(act[k]), case
            assert int(k.sum()) == int(np.asarray(m.flwacc)[r, c]), case       # flow accumulation counts the same cells


def test_upstream_is_iterative_and_follows_inactive_cells():
    # a chain of 5000 cells draining south (code 5): deeper than any recursion limit
    fd = np.full((5000, 1), 5, np.int32)
    assert int(mu.upstream(fd, 4999, 0).sum()) == 5000 and int(mu.upstream(fd, 10, 0).sum()) == 11
    # the reference's mask knows no active cells: all eight neighbours pointing at the centre are taken, the others not
    fd = np.array([[4, 5, 6], [3, 0, 7], [2, 1, 8]], np.int32)
    assert mu.upstream(fd, 1, 1).all()
    assert int(mu.upstream(np.rot90(fd, 2).copy(), 1, 1).sum()) == 1


# ---- argument checks, before anything reaches a device ---------------------------------------------------------------------------------
NT = 48


def _case(ng=2):
    import smash_amd
    from smash_amd import synth
    m = synth.make_mesh(8, 8, ng=ng)
    setup = smash_amd.SetupDT(0, ng, structure="gr-b", ntime_step=NT)
    mesh = smash_amd.MeshDT.from_synth(setup, m)

    class Poisoned(smash_amd.Input_DataDT):
        """Any access to the forcing means the wrapper went on towards the device."""
        def __getattribute__(self, k):
            if k in ("prcp", "pet", "sparse_prcp", "sparse_pet", "qobs"):
                raise AssertionError("the wrapper touched input_data before validating its arguments")
            return object.__getattribute__(self, k)
    return setup, mesh, object.__new__(Poisoned)


def test_input_data_carries_the_two_fields():
    import smash_amd
    setup, mesh, _ = _case()
    inp = smash_amd.Input_DataDT(setup, mesh)
    for a in (inp.mean_prcp, inp.mean_pet):
        assert a.shape == (2, NT) and a.dtype == F and a.flags.f_contiguous and np.all(a == F(-99.0))
    assert inp.mean_prcp is not inp.mean_pet


def test_the_good_arguments_pass_the_check():
    import smash_amd
    mp, me = smash_amd.check_mean_forcing(2, NT)
    assert mp.shape == me.shape == (2, NT) and mp.dtype == F and mp.flags.f_contiguous and np.all(mp == F(-99.0)) and mp is not me
    mine = np.zeros((2, NT), F, order="F")
    out = smash_amd.check_mean_forcing(2, NT, mine, None)
    assert out[0] is mine and out[1].shape == (2, NT)
    assert smash_amd.check_mean_forcing(2, NT, mine, None, pet=False) == (mine, None)
    assert smash_amd.check_mean_forcing(2, NT, None, mine, prcp=False) == (None, mine)


@pytest.mark.parametrize("field", ["mean_prcp", "mean_pet"])
def test_arrays_of_the_wrong_kind(field):
    import smash_amd
    ro = np.zeros((2, NT), F, order="F")
    ro.flags.writeable = False
    for a in (np.zeros((2, NT), np.float64, order="F"), np.zeros((2, NT), F, order="C"), np.zeros((NT, 2), F, order="F"),
              np.zeros((2, NT + 1), F, order="F"), np.zeros((3, NT), F, order="F"), np.zeros((4, NT), F, order="F")[::2], ro,
              [[0.0] * NT] * 2):
        setup, mesh, inp = _case()
        good = np.full((2, NT), 5.0, F, order="F")
        inp.mean_prcp, inp.mean_pet = (a, good) if field == "mean_prcp" else (good, a)
        with pytest.raises(smash_amd.SmashxError, match=f"{field} must be a writeable Fortran-ordered float32 array of shape \\(2, {NT}\\)") as e:
            smash_amd.compute_mean_forcing(setup, mesh, inp)
        assert e.value.code == -1
        assert np.all(good == 5.0)


def test_nothing_asked_for():
    import smash_amd
    with pytest.raises(smash_amd.SmashxError, match="neither prcp nor pet") as e:
        smash_amd.check_mean_forcing(2, NT, prcp=False, pet=False)
    assert e.value.code == -1
    with pytest.raises(smash_amd.SmashxError, match="mean_pet was given but the field is left out") as e:
        smash_amd.check_mean_forcing(2, NT, None, np.zeros((2, NT), F, order="F"), pet=False)
    assert e.value.code == -1


def test_no_gauges_needs_no_device():
    """ng = 0: the reference allocates nothing and loops over nothing; here the two empty arrays are set and the forcing is not read"""
    import smash_amd
    setup, mesh, inp = _case(ng=0)
    mp, me = smash_amd.compute_mean_forcing(setup, mesh, inp)
    assert mp.shape == me.shape == (0, NT) and inp.mean_prcp is mp and inp.mean_pet is me


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
FORCING_HEADER = os.path.join(ROOT, "include", "smashx_forcing.h")


def test_forcing_header_matches_the_binding():
    """include/smashx_forcing.h against _lib.FORCING_PROTOTYPES with the parser and the type rules tests/test_abi_header_cpu.py applies
    to smashx.h and PROTOTYPES; counts taken from the header's own text, so that a declaration the parser skips fails here"""
    import re
    import test_abi_header_cpu as ah
    from smash_amd import _lib
    text = open(FORCING_HEADER).read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    assert [k for k in h["constants"] if k != "SMASHX_FORCING_H"] == []
    assert re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", ah.strip(text)[0], flags=re.M) == ["SMASHX_FORCING_H"]
    assert not re.search(r"\b(struct|enum|typedef)\b", ah.strip(text)[1])
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == 1
    assert sorted(h["functions"]) == sorted(_lib.FORCING_PROTOTYPES) and _lib.FORCING_SYMBOLS == list(_lib.FORCING_PROTOTYPES)
    assert not set(_lib.FORCING_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.SETUP_PROTOTYPES))
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.FORCING_PROTOTYPES[name]
        assert not rptr and restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert [p[:3] for p in h["functions"]["smashx_mean_forcing"][1]] == [
        ("plan", "smashx_plan", True), ("mean_prcp", "float", True), ("mean_pet", "float", True)]
    # the comparison bites: a parameter turned into a scalar is reported
    flat = ah.parse(text.replace("float* mean_pet)", "float mean_pet)"))
    ah.check_type("mean_pet", _lib.FORCING_PROTOTYPES["smashx_mean_forcing"][1][2], *flat["functions"]["smashx_mean_forcing"][1][2][1:],
                  flat, _lib, findings, param=True)
    assert findings and "mean_pet" in findings[0]


def test_smashx_h_brings_the_forcing_header_along():
    """a C caller that includes smashx.h sees the declaration, after the set-up header; no struct changed, so the ABI version stays"""
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    assert hdr.count('#include "smashx_forcing.h"') == 1
    assert hdr.index('#include "smashx_setup.h"') < hdr.index('#include "smashx_forcing.h"')
    assert "#define SMASHX_ABI_VERSION 9" in hdr
    assert "int smashx_mean_forcing(smashx_plan* plan, float* mean_prcp, float* mean_pet);" in open(FORCING_HEADER).read()


def test_symbol_is_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    L = _lib.lib()
    fn = L.smashx_mean_forcing
    restype, argtypes = _lib.FORCING_PROTOTYPES["smashx_mean_forcing"]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert L.smashx_abi_sizes(None) == 9
