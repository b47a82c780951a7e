"""GPU: the forms of the vertical time loops (smash_amd/csrc/sx_kernels.h, sx_ops.h).  The forward and the reverse vertical kernels
prefetch one step ahead into two alternating register sets -- the reverse loop two steps per turn inside a block of SX_HIK = 8
steps, the forward loop four -- and a wavefront none of whose lanes is in a data gap at a step takes the gap-free form of that step.
None of it may change a bit, so every case here is compared with oracle/pyoracle.run on the same inputs (the oracle is pinned to the
reference bit for bit, tests/test_oracle_golden.py), never with another run of the library:
  exact-libm build  bit-identical discharge, cost, final states and every gradient field (the last test runs this module under
                    SMASHX_EXACT_LIBM=1; so does any run of the module with that variable set);
  default build     within golden_util.tol, output by output, as tests/test_gpu_parity.py does -- of the reference's own flag-to-flag
                    noise on that output FOR THESE INPUTS (tests/golden/vertical_forms/noise.npz, recorded by
                    tests/golden/vertical_forms/make_noise.py the way make_golden.py records it for the fixtures).  The noise stored in
                    a fixture belongs to its 96 steps: over 3 to 17 steps the reference's two builds differ by 5e-5 .. 2e-4 on cp_b
                    where they differ by 6e-6 over 96 (and the default build differs from the oracle by 2e-5 .. 1e-4 there).
Inputs (tests/vertical_forms_cases.py): mesh, parameters and options of gr_b_16x16x96_nse_gaps (gr-a, gr-c: the 16x16x96 fixtures; gr-d
has no fixture of that size, its smallest one, 12x12x48, stands in), the forcing cut to the step counts at which an unrolled two-set
loop can go wrong."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from smash_amd import synth

import vertical_forms_cases as vc
from vertical_forms_cases import BASE, NTS, OTHERS, OTHER_NTS, PATTERNS

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

SYNTH_LAYOUT = dict(compact=True, prcp_factor=0.1, pet_ratio=synth._pet_tables()[1], pet_hour0=0)
WAVE = 64                              # lanes of a wavefront: plan cells [64 w, 64 w + 64) march together (the vertical kernels' k)


@functools.lru_cache(maxsize=None)
def _noise():
    return dict(np.load(os.path.join(gu.GOLDEN_DIR, "vertical_forms", "noise.npz")))


@functools.lru_cache(maxsize=None)
def _case(name, nt, pattern):
    """The case and the oracle's forward and adjoint results for it (computed once per case, shared by the variants, never modified)."""
    from oracle import pyoracle
    g = vc.make(name, nt, pattern)
    run = functools.partial(pyoracle.run, g.structure, g.mesh, g.dt, g.prcp, g.pet, g.qobs, g.params, g.states, **g.opts)
    g.oracle = vc.outputs(g.structure, run(), run(adjoint=True))
    g.noise_cut = {k: float(_noise()[vc.key(name, nt, pattern, k)]) for k in g.oracle}
    g.pattern = pattern
    return g


def _gap_free(g, rows, cols):
    """[wavefront][step]: True where the wavefront takes the gap-free form -- no lane of it has a negative rain value (compact
    layout: the gap count) or a negative PET (compact: a negative day) at that step.  rows / cols: Solver.cell_order()."""
    ok = (g.prcp[rows, cols, :] >= 0) & (g.pet[rows, cols, :] >= 0)               # (cell, step)
    return np.array([ok[w:w + WAVE].all(axis=0) for w in range(0, len(rows), WAVE)])


def _check_forms(g, pattern, form):
    """The gap pattern reaches the forms it is meant for."""
    nt = g.nt
    if pattern == "none":
        assert form.all()
    elif pattern == "own":
        if nt >= 17 and g.name == BASE:
            assert (~form).any() and form.any(), "the fixture's own gaps send some wavefront-steps each way"
    elif pattern == "all_at_one_step":
        assert not form[:, nt // 2].any() and np.delete(form, nt // 2, axis=1).all()
    else:
        hit = np.nonzero(~form.all(axis=1))[0]
        assert len(hit) == 1, hit                   # one wavefront leaves the gap-free form ...
        assert sorted(np.nonzero(~form[hit[0]])[0]) == g.gap_steps          # ... at the ends of the loop and nowhere else


def _same(a, b):
    """bit-identical up to which NaN it is"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _within(a, b, bar):
    """rel-L2 over the finite values <= bar, the others (a criterion over one or two steps can be 0 / 0) the same"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    fin = np.isfinite(b)
    if not (np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], b[~fin], equal_nan=True)):
        return np.inf, False
    e = gu.rel_l2(a[fin], b[fin])
    return e, e <= bar


def _compare(g, kw, pattern, monkeypatch, hi_tape=None):
    import smash_amd
    from smash_amd import _lib
    from test_gpu_parity import _types
    if hi_tape is not None:
        monkeypatch.setenv("SMASHX_HI_TAPE", str(hi_tape))
    # forward (the untaped kernel) ...
    setup, mesh, inp, par, sta, out = _types(g, **dict(kw))
    sol = inp._smashx_solver
    form = _gap_free(g, *sol.cell_order())
    _check_forms(g, pattern, form)
    if "layout" in kw:
        assert sol.forcing_info()["layout"].startswith("compact")
    smash_amd.forward(setup, mesh, inp, par, inp._bgd[0], sta, inp._bgd[1], out, np.float32(0))
    # ... and forward taped + reverse, on a plan of its own
    setup, mesh, inp, par, sta, out_b = _types(g, **dict(kw))
    par_b, sta_b = par.copy(), sta.copy()
    smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), out_b,
                        out_b.copy(), np.float32(0), np.float32(1))
    got = vc.outputs(g.structure, dict(qsim=out.qsim, cost=out.cost, fstates={k: getattr(out.fstates, k) for k in gu.STRUCT_STATES[g.structure]}),
                     dict(qsim=out_b.qsim, cost=out_b.cost, parameters_b={k: getattr(par_b, k) for k in gu.STRUCT_PARAMS[g.structure]},
                          states_b={k: getattr(sta_b, k) for k in gu.STRUCT_STATES[g.structure]}))
    if _lib.EXACT:
        bad = [k for k in got if not _same(got[k], g.oracle[k])]
        assert not bad, bad
        return
    report = {}
    for k, a in got.items():
        b, noise = g.oracle[k], g.noise_cut[k]
        if k.startswith("cost") and np.isfinite(b):      # absolute, with golden_util.tol_cost's floor
            e, bar = abs(float(a) - float(b)), gu.tol_cost(noise, float(b))
            ok = e <= bar
        else:
            bar = gu.tol_fstate("hlr", noise) if k == "fstates.hlr" else gu.tol(noise)
            e, ok = _within(a, b, bar)
        report[k] = (float(e), bar, bool(ok))
    print(g.name, g.nt, pattern, kw.get("chunk_steps"), {k: f"{v[0]:.1e} ({v[1]:.0e})" for k, v in report.items()})
    bad = {k: v for k, v in report.items() if not v[2]}
    assert not bad, bad


def _kw(layout, chunk=0):
    return dict(chunk_steps=chunk, **({"layout": dict(SYNTH_LAYOUT)} if layout == "compact" else {}))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", ["compact", "fp32"])
@pytest.mark.parametrize("hi_tape", [0, 1])
@pytest.mark.parametrize("nt", NTS)
def test_gr_b_step_counts(nt, hi_tape, layout, pattern, monkeypatch):
    _compare(_case(BASE, nt, pattern), _kw(layout), pattern, monkeypatch, hi_tape)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", ["compact", "fp32"])
@pytest.mark.parametrize("hi_tape", [0, 1])
def test_gr_b_last_storage_chunk_of_one_step(hi_tape, layout, pattern, monkeypatch):
    """33 steps in storage chunks of 16: the last chunk has one step, and in the chunks before it the reverse blocks start on the
    second register set."""
    _compare(_case(BASE, 33, pattern), _kw(layout, 16), pattern, monkeypatch, hi_tape)


@pytest.mark.parametrize("name", OTHERS)
@pytest.mark.parametrize("layout", ["compact", "fp32"])
@pytest.mark.parametrize("nt", OTHER_NTS)
def test_other_structures(nt, layout, name, monkeypatch):
    """gr-a, gr-c and gr-d, one gap pattern each way: the fixture's own gaps where it has some, else one cell at the ends."""
    pattern = vc.other_pattern(name, nt)
    _compare(_case(name, nt, pattern), _kw(layout), pattern, monkeypatch)
    _compare(_case(name, nt, "none"), _kw(layout), "none", monkeypatch)


@pytest.mark.parametrize("chunk", [16, 32])
@pytest.mark.parametrize("layout", ["compact", "fp32"])
def test_chunking_does_not_change_results(layout, chunk, monkeypatch):
    """The whole fixture (96 steps) in storage chunks of 16 and 32 steps, each against the oracle."""
    _compare(_case(BASE, 96, "own"), _kw(layout, chunk), "own", monkeypatch)
    _compare(_case(BASE, 96, "one_cell_at_the_ends"), _kw(layout, chunk), "one_cell_at_the_ends", monkeypatch)


def test_exact_build_is_bit_identical_on_the_vertical_forms():
    """Every case above under the exact-libm build (a separate process: the library is chosen at import time)."""
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not test_exact_build"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    sys.stdout.write(r.stdout[-3000:])
    n = 4 * 2 * 2 * len(NTS) + 4 * 2 * 2 + len(OTHERS) * 2 * len(OTHER_NTS) + 2 * 2
    assert r.returncode == 0 and f"{n} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
