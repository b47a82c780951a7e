"""CPU: the interception adjustment (adjust_interception_store, mw_interception_store.f90:19-160) -- the numpy restatement against the
fixtures recorded from the compiled reference (exact equality of fp32 bit patterns: same IEEE operations, same order, discrete
result), smash_amd.day_index against hand-written dates, every argument error of check_adjust_interception raised before anything
reaches a device, and the new entry point declared on both sides of the ABI.  Runs without a GPU."""
import os

import numpy as np
import pytest

import interception_util as iu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement is the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(iu.CASES))
def test_numpy_restatement_equals_the_reference(name):
    g, day, nday, ci = iu.load(name)
    assert day.shape == (g.nt,) and day[0] == 1 and day[-1] == nday
    p, e, rows, cols = iu.active_columns(g)
    mine, _ = iu.adjust(p, e, day)
    assert mine.dtype == np.float32
    assert np.array_equal(_bits(mine), _bits(ci[rows, cols]))


@pytest.mark.parametrize("name", sorted(iu.CASES))
def test_fixture_shows_something(name):
    """at least 5 distinct capacities on active cells, inactive cells untouched by the reference"""
    g, day, nday, ci = iu.load(name)
    act = np.asarray(g.mesh.active_cell) == 1
    assert np.unique(ci[act]).size >= 5
    assert np.all(np.isin(_bits(ci[act]), _bits(iu.candidates())))
    assert np.all(ci[~act] == np.float32(-7.0))


def test_fixture_properties():
    """what makes the cases worth recording: exact ties between the two best candidates and -99 gaps in the synthetic ones, partial
    first and last days in the 17:00 run"""
    for name, ties, gaps in (("gr_b_16x16x96_nse_gaps", True, True), ("gr_c_32x32x240_d8_ragged", True, True),
                             ("gr_a_cance_28x28x1440", False, False)):
        g, day, nday, ci = iu.load(name)
        p, e, rows, cols = iu.active_columns(g)
        _, diff = iu.adjust(p, e, day)
        assert (iu.exact_ties(diff) > 0) == ties, name
        assert bool(np.any(p == -99.0) or np.any(e == -99.0)) == gaps, name
    _, day, nday, _ = iu.load("gr_b_16x16x96_nse_gaps__start17")
    counts = np.bincount(day)[1:]
    assert nday == 5 and counts[0] == 6 and counts[-1] == 18 and np.all(counts[1:-1] == 24)     # 18:00 .. 23:00 | ... | 00:00 .. 17:00


def test_candidates():
    c = iu.candidates()
    assert c.dtype == np.float32 and c.size == 49
    assert c[0] == np.float32(0.1) and c[-1] == np.float32(0.1) + np.float32(48.0) * np.float32(0.1)


# ---- day_index ----------------------------------------------------------------------------------------------------------------------
def test_day_index_midnight_start():
    import smash_amd
    d = smash_amd.day_index("2014-09-15 00:00", "2014-09-17 00:00", 3600)
    # steps 01:00 .. 23:00 of the 15th (23), the whole 16th (24), 00:00 of the 17th (1)
    assert d.dtype == np.int32 and d.shape == (48,)
    assert d.tolist() == [1] * 23 + [2] * 24 + [3]


def test_day_index_start_at_17():
    import smash_amd
    d = smash_amd.day_index("2014-09-15 17:00", "2014-09-17 05:00", 3600)
    # 18:00 .. 23:00 (6), the 16th (24), 00:00 .. 05:00 of the 17th (6)
    assert d.tolist() == [1] * 6 + [2] * 24 + [3] * 6


def test_day_index_month_boundary():
    import smash_amd
    d = smash_amd.day_index("2015-02-28 12:00", "2015-03-01 12:00", 3600)      # 2015 is not a leap year
    assert d.tolist() == [1] * 11 + [2] * 13
    d = smash_amd.day_index("2016-02-28 12:00", "2016-03-01 12:00", 3600)      # 2016 is: the 29th lies in between
    assert d.tolist() == [1] * 11 + [2] * 24 + [3] * 13


def test_day_index_half_hourly():
    import smash_amd
    d = smash_amd.day_index(np.datetime64("2014-09-15T23:00"), np.datetime64("2014-09-16T01:00"), 1800)
    # 23:30 | 00:00 00:30 01:00
    assert d.tolist() == [1, 2, 2, 2]
    d = smash_amd.day_index("2014-09-15 00:00", "2014-09-16 00:20", 1800)      # an end that is no whole step away: 48 steps
    assert d.shape == (48,) and d[-2] == 1 and d[-1] == 2


def test_day_index_matches_the_recorded_ones():
    import smash_amd
    for name in iu.CASES:
        z = np.load(os.path.join(iu.DIR, name + ".npz"))
        start = np.datetime64(str(z["start_time"]).replace(" ", "T"))
        nt = z["day_index"].size
        d = smash_amd.day_index(start, start + np.timedelta64(3600 * nt, "s"), 3600.0)
        assert np.array_equal(d, z["day_index"]), name


def test_day_index_errors():
    import smash_amd
    for args in (("2014-09-15 00:00", "2014-09-15 00:30", 3600), ("2014-09-15 00:00", "2014-09-16 00:00", 0),
                 ("2014-09-15 00:00", "2014-09-16 00:00", 0.5)):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.day_index(*args)
        assert e.value.code == -1


# ---- argument checks, before anything reaches a device ---------------------------------------------------------------------------------
NT = 48


def _case(structure="gr-b"):
    import smash_amd
    from smash_amd import synth
    m = synth.make_mesh(8, 8, ng=2)
    setup = smash_amd.SetupDT(0, 2, structure=structure, ntime_step=NT)
    mesh = smash_amd.MeshDT.from_synth(setup, m)

    class Poisoned(smash_amd.Input_DataDT):
        """Any access to the forcing means the wrapper went on towards the device."""
        def __getattribute__(self, k):
            if k in ("prcp", "pet", "sparse_prcp", "sparse_pet", "qobs"):
                raise AssertionError("the wrapper touched input_data before validating its arguments")
            return object.__getattribute__(self, k)
    return setup, mesh, object.__new__(Poisoned), smash_amd.ParametersDT(mesh)


GOOD = np.repeat(np.arange(1, 3), 24)


def _raises(code, match, day=GOOD, nday=2, structure="gr-b", ci="keep"):
    import smash_amd
    setup, mesh, inp, par = _case(structure)
    if not isinstance(ci, str):
        par.ci = ci
    before = np.array(par.ci, copy=True) if isinstance(par.ci, np.ndarray) else None
    with pytest.raises(smash_amd.SmashxError, match=match) as e:
        smash_amd.adjust_interception_store(setup, mesh, inp, par, nday, day)
    assert e.value.code == code
    if before is not None and isinstance(par.ci, np.ndarray) and par.ci.shape == before.shape:
        assert np.array_equal(par.ci, before)


def test_the_good_arguments_pass_the_check():
    import smash_amd
    nday, day, ci = smash_amd.check_adjust_interception("gr-b", 8, 8, NT, 2, GOOD)
    assert nday == 2 and day.dtype == np.int32 and day.flags.c_contiguous and np.array_equal(day, GOOD)
    assert ci.shape == (8, 8) and ci.dtype == np.float32 and ci.flags.f_contiguous
    mine = np.full((8, 8), 3.0, np.float32, order="F")
    assert smash_amd.check_adjust_interception("gr-c", 8, 8, NT, np.int64(2), GOOD.astype(np.int64), mine)[2] is mine


@pytest.mark.parametrize("structure", ["gr-a", "gr-d", "vic-a"])
def test_structure_without_interception_store(structure):
    _raises(-2, "no interception store", structure=structure)


def test_day_index_not_an_integer_vector():
    _raises(-1, "1-D integer array", day=GOOD.astype(np.float32))
    _raises(-1, "1-D integer array", day=GOOD.reshape(2, 24))
    _raises(-1, "1-D integer array", day=None)


def test_day_index_wrong_length():
    _raises(-1, "47 entries", day=GOOD[:-1])
    _raises(-1, "49 entries", day=np.append(GOOD, 2))


def test_day_index_does_not_start_at_one():
    _raises(-1, "start at 1", day=GOOD + 1, nday=3)
    _raises(-1, "start at 1", day=GOOD - 1, nday=1)


def test_day_index_not_monotonic():
    d = GOOD.copy(); d[30] = 1
    _raises(-1, "steps of 0 or 1", day=d)
    d = GOOD.copy(); d[24:] = 3
    _raises(-1, "steps of 0 or 1", day=d, nday=3)


def test_day_index_does_not_end_at_nday():
    _raises(-1, "ends at day 2", nday=3)
    _raises(-1, "ends at day 2", nday=1)
    _raises(-1, "nday must be an integer", nday=2.0)


def test_ci_plane_of_the_wrong_kind():
    import smash_amd
    for ci in (np.zeros((8, 8), np.float64, order="F"), np.zeros((8, 7), np.float32, order="F"), np.zeros((16, 8), np.float32)[::2],
               [[0.0] * 8] * 8):
        with pytest.raises(smash_amd.SmashxError, match="Fortran-ordered float32") as e:
            smash_amd.check_adjust_interception("gr-b", 8, 8, NT, 2, GOOD, ci)
        assert e.value.code == -1


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
SETUP_HEADER = os.path.join(ROOT, "include", "smashx_setup.h")


def test_setup_header_matches_the_binding():
    """include/smashx_setup.h against _lib.SETUP_PROTOTYPES with the parser and the type rules tests/test_abi_header_cpu.py applies to
    smashx.h and PROTOTYPES; counts taken from the header's own text, so that a declaration the parser skips fails here"""
    import ctypes as C
    import re
    import test_abi_header_cpu as ah
    from smash_amd import _lib
    text = open(SETUP_HEADER).read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    assert [k for k in h["constants"] if k != "SMASHX_SETUP_H"] == []
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == 1
    assert sorted(h["functions"]) == sorted(_lib.SETUP_PROTOTYPES) and _lib.SETUP_SYMBOLS == list(_lib.SETUP_PROTOTYPES)
    assert not set(_lib.SETUP_PROTOTYPES) & set(_lib.PROTOTYPES)
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.SETUP_PROTOTYPES[name]
        assert not rptr and restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert [p[:3] for p in h["functions"]["smashx_adjust_interception"][1]] == [
        ("plan", "smashx_plan", True), ("nday", "int", False), ("day_index", "int", True), ("ci", "float", True)]
    # the comparison bites: a widened parameter is reported
    wide = ah.parse(text.replace("int nday,", "long long nday,"))
    ah.check_type("nday", _lib.SETUP_PROTOTYPES["smashx_adjust_interception"][1][1], *wide["functions"]["smashx_adjust_interception"][1][1][1:],
                  wide, _lib, findings, param=True)
    assert findings and "nday" in findings[0]
    assert C.c_int is _lib.SETUP_PROTOTYPES["smashx_adjust_interception"][1][1]


def test_smashx_h_brings_the_setup_header_along():
    """a C caller that includes smashx.h sees the declaration; no struct changed, so the ABI version stays"""
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    assert hdr.count('#include "smashx_setup.h"') == 1
    assert "#define SMASHX_ABI_VERSION 9" in hdr
    assert "int smashx_adjust_interception(smashx_plan* plan, int nday, const int* day_index, float* ci);" in open(SETUP_HEADER).read()


def test_symbol_is_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    L = _lib.lib()
    fn = L.smashx_adjust_interception
    restype, argtypes = _lib.SETUP_PROTOTYPES["smashx_adjust_interception"]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert L.smashx_abi_sizes(None) == 9
