"""CPU: the ensemble entry point (smashx_multiple_run, compute_multiple_run of mw_multiple_run.f90:68-119) is exported and
declared, and the Python wrappers refuse every malformed input with SmashxError(E_ARG) BEFORE anything reaches a device: these
tests run without a GPU (validation first, device second)."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbol_is_exported_and_declared():
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smashx.h")).read()
    for sym in ("smashx_multiple_run", "smashx_multiple_run_info"):
        assert sym + "(" in hdr
        assert sym in _lib.SYMBOLS
        assert hasattr(_lib.lib(), sym)
    assert "#define SMASHX_ABI_VERSION 9" in hdr
    assert _lib.lib().smashx_abi_sizes(None) == 9


def _case(structure="gr-a", nt=6):
    import smash_amd
    from smash_amd import synth
    m = synth.make_mesh(8, 8, ng=2)
    setup = smash_amd.SetupDT(0, 2, structure=structure, ntime_step=nt)
    mesh = smash_amd.MeshDT.from_synth(setup, m)

    class Poisoned(smash_amd.Input_DataDT):
        """Any access to the forcing means the wrapper went on towards the device."""
        def __getattribute__(self, k):
            if k in ("prcp", "pet", "sparse_prcp", "sparse_pet", "qobs"):
                raise AssertionError("the wrapper touched input_data before validating its arguments")
            return object.__getattribute__(self, k)
    inp = object.__new__(Poisoned)
    par, sta = smash_amd.ParametersDT(mesh), smash_amd.StatesDT(mesh)
    out = smash_amd.OutputDT(setup, mesh)
    return setup, mesh, inp, par, sta, out


def _call(sample, ind, res_cost="auto", res_qsim="none", structure="gr-a"):
    import smash_amd
    setup, mesh, inp, par, sta, out = _case(structure)
    S = sample.shape[1] if isinstance(sample, np.ndarray) and sample.ndim == 2 else 1
    if isinstance(res_cost, str):
        res_cost = np.zeros(S, np.float32)
    if isinstance(res_qsim, str):
        res_qsim = np.zeros(0, np.float32)
    return smash_amd.compute_multiple_run(setup, mesh, inp, par, sta, out, sample, ind, res_cost, res_qsim)


def _f(a):
    return np.asfortranarray(a, dtype=np.float32)


GOOD = _f(np.full((2, 3), 100.0))

BAD = {
    "index 0": (GOOD, [0, 2]),
    "index 25": (GOOD, [2, 25]),
    "repeated index": (GOOD, [2, 2]),
    "field the structure does not use (ci in gr-a)": (GOOD, [1, 2]),
    "state the structure does not use (hst in gr-a)": (GOOD, [2, 20]),
    "S < 1": (_f(np.zeros((2, 0))), [2, 4]),
    "index list shorter than sample": (GOOD, [2]),
    "float index list": (GOOD, np.array([2.0, 4.0])),
    "sample 1-D": (np.zeros(3, np.float32), [2]),
    "sample float64": (np.asfortranarray(np.full((2, 3), 100.0)), [2, 4]),
    "sample C order": (np.ascontiguousarray(np.full((2, 3), 100.0, np.float32)), [2, 4]),
    "sample not an array": ([[1.0, 2.0]], [2]),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_malformed_input_is_refused_before_the_device(what):
    import smash_amd
    from smash_amd import _lib
    sample, ind = BAD[what]
    with pytest.raises(smash_amd.SmashxError) as e:
        _call(sample, ind)
    assert e.value.code == _lib.E_ARG, what


@pytest.mark.parametrize("what", ["res_cost None", "res_cost shape", "res_cost dtype", "res_qsim shape", "res_qsim C order", "res_qsim dtype"])
def test_malformed_outputs_are_refused_before_the_device(what):
    import smash_amd
    from smash_amd import _lib
    ng, nt, S = 2, 6, 3
    rc, rq = np.zeros(S, np.float32), np.zeros((ng, nt, S), np.float32, order="F")
    if what == "res_cost None":
        rc = None
    elif what == "res_cost shape":
        rc = np.zeros(S + 1, np.float32)
    elif what == "res_cost dtype":
        rc = np.zeros(S, np.float64)
    elif what == "res_qsim shape":
        rq = np.zeros((nt, ng, S), np.float32, order="F")
    elif what == "res_qsim C order":
        rq = np.zeros((ng, nt, S), np.float32, order="C")
    elif what == "res_qsim dtype":
        rq = np.zeros((ng, nt, S), np.float64, order="F")
    with pytest.raises(smash_amd.SmashxError) as e:
        _call(GOOD, [2, 4], rc, rq)
    assert e.value.code == _lib.E_ARG, what


def test_dict_form_checks_names_and_lengths():
    import smash_amd
    from smash_amd import _lib
    setup, mesh, inp, par, sta, out = _case()
    for sample in ({}, {"nope": [1.0]}, {"cp": [1.0, 2.0], "cft": [1.0]}, {"ci": [1.0]}):
        with pytest.raises(smash_amd.SmashxError) as e:
            smash_amd.multiple_run(setup, mesh, inp, par, sta, sample)
        assert e.value.code == _lib.E_ARG, sample


def test_field_table_matches_the_structures():
    """The wrapper's table of fields per structure is the one the tests' golden helper and md_constant's order give."""
    import golden_util as gu
    from smash_amd import solver, synth
    assert solver.FIELD_NAMES == tuple(synth.PARAM_NAMES) + tuple(synth.STATE_NAMES) and len(solver.FIELD_NAMES) == 24
    for st in gu.STRUCT_PARAMS:
        assert set(solver.STRUCTURE_FIELDS[st]) == set(gu.STRUCT_PARAMS[st]) | set(gu.STRUCT_STATES[st]), st


def test_valid_input_reaches_the_device_layer():
    """The same call with well-formed arguments gets past validation: it goes on to the forcing (this file's poisoned
    input_data trips) -- so the refusals above are not vacuous."""
    with pytest.raises(AssertionError, match="touched input_data"):
        _call(GOOD, [2, 4], res_qsim=np.zeros((2, 6, 3), np.float32, order="F"))
