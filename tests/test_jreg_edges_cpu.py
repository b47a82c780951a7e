"""CPU: the regulariser cases of tests/jreg_cases.py (edges of grid shape, mask and sum length).  The plain-C oracle -- the reference
of tests/test_gpu_jreg_edges.py -- equals what the compiled reference recorded in tests/golden/jreg_edges/jreg_edges.npz
(tests/golden/make_jreg_edges.py) BIT FOR BIT: cost, cost_jobs, cost_jreg, cost_d and every gradient plane; a plane the fixture does
not hold is zero.  Where oracle/_ref is built the fixture is also held to a fresh run of the compiled reference.  The routing
schedule accepts every mesh, and the sums are as long as the table of jreg_cases says."""
import os

import numpy as np
import pytest

import jreg_cases as jc
from oracle import pyoracle, refbind
from test_mesh_cpu import _probe

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jreg_edges", "jreg_edges.npz")
CASES = [(cid, w) for cid in jc.IDS for w in jc.WEIGHTINGS]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, pre):
    """names under which the float32 bits of got differ from the fixture's, or that only one side holds"""
    want = {k: v for k, v in want.items() if k.startswith(pre)}
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or got[k].shape != want[k].shape
                  or not np.array_equal(_bits(got[k]), _bits(want[k])))


@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case_and_nothing_else(fixture):
    assert {k.rsplit(".", 1)[0] for k in fixture} == {f"{cid}.{w}" for cid, w in CASES}
    assert all(v.dtype == np.float32 for v in fixture.values())


@pytest.mark.parametrize("cid,w", CASES)
def test_oracle_equals_the_recorded_reference(fixture, cid, w):
    bad = _same(jc.recorded(jc.build(cid, w), pyoracle.run), fixture, f"{cid}.{w}.")
    assert not bad, bad


@pytest.mark.skipif(not refbind.available(False), reason="oracle/_ref/libsmash_ref.so not built")
@pytest.mark.parametrize("cid,w", CASES)
def test_fixture_equals_a_fresh_run_of_the_reference(fixture, cid, w):
    bad = _same(jc.recorded(jc.build(cid, w), refbind.run), fixture, f"{cid}.{w}.")
    assert not bad, bad


@pytest.mark.parametrize("cid", jc.IDS)
def test_schedule_accepts_the_mesh(cid):
    m = jc.make_mesh(cid)
    assert _probe(m)["cells"] == m.nac == int(jc.active(cid).sum())


def test_chain_lengths_of_the_table():
    """terms of a running sum = optimised fields of its group x nrow x ncol: below, at and above 64 and 256 terms, a multiple of
    64 that is none of 256, an empty sum"""
    for cid in jc.IDS:
        (nrow, ncol), _, _, _, chains = jc.CASES[cid.replace("_raw", "")]
        op, os_ = jc.optimised(cid)
        g = jc.build(cid)
        assert np.array_equal(g.opts["optim_parameters"], op) and np.array_equal(g.opts["optim_states"], os_)
        assert (g.mesh.nrow, g.mesh.ncol) == (nrow, ncol)
        assert (int(op.sum()) * nrow * ncol, int(os_.sum()) * nrow * ncol) == chains, cid
        assert len(g.opts["jreg_fun"]) == 4               # eight running sums
    lengths = {n for c in jc.CASES.values() for n in c[4]}
    assert {0, 9, 37, 63, 64, 65, 255, 256, 257, 320, 512, 513} <= lengths


def test_masks_hold_the_edges_they_are_named_for():
    def neighbours(a):
        p = np.pad(a, 1)
        return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]
    a = jc.active("checker_6x11")
    assert not np.any(neighbours(a)[a == 1])                          # every 4-neighbour of an active cell is inactive
    a = jc.active("islands_6x11")
    assert a[2, 4] == 1 and neighbours(a)[2, 4] == 0 and neighbours(a)[5, 0] == 0      # two isolated cells
    a = jc.active("holes_7x19")
    assert a[3, 9] == 0 and neighbours(a)[3, 9] == 4                  # a hole
    a = jc.active("serpent_9x5")
    assert a.sum() == 29 and np.all(neighbours(a)[a == 1] <= 3)
    assert jc.active("one_cell_3x3").sum() == 1
    # the background differs from the fields on every cell of every optimised field but ci, which the perturbation leaves alone
    g = jc.build("holes_7x19")
    for k in ("cp", "cst", "lr"):
        assert np.all(g.params[k] != g.opts["params_bgd"][k]), k
    for k in ("hp", "hst"):
        assert np.all(g.states[k] != g.opts["states_bgd"][k]), k
