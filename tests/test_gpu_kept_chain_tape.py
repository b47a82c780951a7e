"""GPU: the kept tape of the chained routing launches, the circular routing tape and the early adjoint chain.

An adjoint sweep over C > 1 storage chunks tapes hr_imd of the chained routing groups in the FIRST pass into rows of its own
(SMASHX_KEEP_CHAIN_TAPE, default on); the recomputation of a chunk then runs neither the copy into the staging rows nor the chained
forward launch, and the chained adjoint launch reads the kept rows -- on staging rows it is queued before the chunk is recomputed.
The routing tape itself is indexed by (time block + stage) mod the rows of the chunk (SMASHX_HR_SKEW) and needs no extra rows.
All of it moves work and addresses only: every output must be BIT-IDENTICAL with the switches off and to the single-chunk sweep.

Chained rounds need three routing rounds (rounds >= 1, at least two of them).  At the smallest group size (64) only the 64 x 64
fixture has them; the two small fixtures have two rounds, so they run with SMASHX_CHAIN_FROM=0, which chains both (every routing
group then belongs to the chained launch: the kept tape is the whole routing tape).  Chunk lengths are multiples of 16 steps: the
96-step fixture cannot be cut into 4 chunks, it runs with 3 and 6."""
import numpy as np
import pytest

import golden_util as gu
from test_gpu_parity import _types

pytestmark = pytest.mark.gpu

# name, group_size, SMASHX_CHAIN_FROM (None = default), [(chunk_steps, C, last chunk ragged)]
FIXTURES = {
    "gr_b_64x64x720_nse": (64, None, [(240, 3, False), (192, 4, True)]),
    "gr_c_32x32x240_d8_ragged": (64, "0", [(80, 3, False), (64, 4, True)]),
    "gr_b_20x20x96_d8": (64, "0", [(32, 3, False), (16, 6, False)]),
}
CASES = [pytest.param(n, chunk, C, stage, id=f"{n}-{chunk}-stage{stage}")
         for n, (_, _, chunks) in FIXTURES.items() for chunk, C, _ in chunks for stage in ("0", "1")]


def _sweeps(g, nsweeps=1, **kw):
    """nsweeps adjoint sweeps on ONE plan; returns [(out, par_b, sta_b)] per sweep and the plan's timing after the last."""
    import smash_amd
    setup, mesh, inp, par, sta, out = _types(g, **kw)
    res = []
    for _ in range(nsweeps):
        par_b, sta_b, o = par.copy(), sta.copy(), out.copy()
        smash_amd.forward_b(setup, mesh, inp, par, par_b, inp._bgd[0], par.copy(), sta, sta_b, inp._bgd[1], sta.copy(), o,
                            o.copy(), np.float32(0), np.float32(1))
        res.append((o, par_b, sta_b))
    return res, inp._smashx_solver.timing()


def _same(g, a, b, what):
    assert np.array_equal(a[0].qsim, b[0].qsim), what
    assert a[0].cost == b[0].cost, (what, a[0].cost, b[0].cost)
    for k in gu.STRUCT_PARAMS[g.structure]:
        assert np.array_equal(getattr(a[1], k), getattr(b[1], k)), (what, k)
    for k in gu.STRUCT_STATES[g.structure]:
        assert np.array_equal(getattr(a[2], k), getattr(b[2], k)), (what, k)


def _within_golden_bar(g, r):
    out, par_b, sta_b = r
    for i in range(g.mesh.ng):
        assert gu.rel_l2(out.qsim[i], g.adj["qsim"][i]) <= gu.tol(g.noise["qsim"][i]), i
    assert abs(out.cost - g.adj["cost"]) <= gu.tol_cost(g.noise["cost"], g.adj["cost"])
    for k in gu.STRUCT_PARAMS[g.structure]:
        e = gu.rel_l2(getattr(par_b, k), g.adj["parameters_b"][k])
        assert e <= gu.tol(g.noise["parameters_b"][k]), (k, e)
    for k in gu.STRUCT_STATES[g.structure]:
        e = gu.rel_l2(getattr(sta_b, k), g.adj["states_b"][k])
        assert e <= gu.tol(g.noise["states_b"][k]), (k, e)


_single = {}


def _single_chunk(name, monkeypatch):
    """The single-chunk sweep of a fixture at the group size and chained rounds of its cases: computed once, shared, left unchanged."""
    if name not in _single:
        group, chain_from, _ = FIXTURES[name]
        if chain_from is not None:
            monkeypatch.setenv("SMASHX_CHAIN_FROM", chain_from)
        g = gu.load(name)
        (r,), tm = _sweeps(g, group_size=group)
        assert tm["n_chunks"] == 1 and tm["n_chained_groups"] > 0, tm
        _within_golden_bar(g, r)
        _single[name] = (g, r)
    return _single[name]


@pytest.mark.parametrize("name,chunk,C,stage", CASES)
def test_kept_chain_tape_and_circular_tape_are_bit_identical(name, chunk, C, stage, monkeypatch):
    group, chain_from, _ = FIXTURES[name]
    g, single = _single_chunk(name, monkeypatch)
    if chain_from is not None:
        monkeypatch.setenv("SMASHX_CHAIN_FROM", chain_from)
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", stage)
    kw = dict(chunk_steps=chunk, pipe_steps=0, group_size=group)

    monkeypatch.setenv("SMASHX_KEEP_CHAIN_TAPE", "1")
    monkeypatch.setenv("SMASHX_HR_SKEW", "1")
    (on, again), tm_on = _sweeps(g, nsweeps=2, **kw)
    monkeypatch.setenv("SMASHX_KEEP_CHAIN_TAPE", "0")
    (off,), tm_off = _sweeps(g, **kw)
    monkeypatch.setenv("SMASHX_KEEP_CHAIN_TAPE", "1")
    monkeypatch.setenv("SMASHX_HR_SKEW", "0")
    (plain,), tm_plain = _sweeps(g, **kw)

    # not vacuous: the plan is cut as the case says, it has chained rounds, the recomputed chunks run no chained forward launch
    for tm in (tm_on, tm_off, tm_plain):
        assert tm["n_chunks"] == C and tm["n_chained_groups"] > 0, tm
        assert tm["chain_staged"] == int(stage), tm
    assert tm_on["route_fwd_chained_launches"] == C, tm_on
    assert tm_plain["route_fwd_chained_launches"] == C, tm_plain
    assert tm_off["route_fwd_chained_launches"] == 2 * C - 1, tm_off
    assert tm_on["route_adj_chained_launches"] == tm_off["route_adj_chained_launches"] == C
    assert tm_on["device_bytes"] <= tm_plain["device_bytes"], (tm_on["device_bytes"], tm_plain["device_bytes"])
    assert tm_on["device_bytes"] > tm_off["device_bytes"]        # (the kept rows are really there)

    _same(g, on, off, "kept tape on / off")
    _same(g, on, plain, "routing tape by super-step / by time block")
    _same(g, on, single, "storage chunks / single chunk")
    _same(g, on, again, "second sweep on the same plan")
    _within_golden_bar(g, on)


def test_last_chunk_of_the_ragged_cases_is_short():
    """The cases marked ragged really end in a shorter chunk (chunk lengths are what the plan makes of chunk_steps: multiples of 16,
    balanced)."""
    for name, (_, _, chunks) in FIXTURES.items():
        nt = gu.load(name).nt
        for chunk, C, ragged in chunks:
            assert (nt + chunk - 1) // chunk == C and (nt % chunk != 0) == ragged, (name, chunk)
    assert any(r for _, _, chunks in FIXTURES.values() for _, _, r in chunks)


def test_tiles_keep_todays_path_with_the_switch_on(monkeypatch):
    """A tiled plan (boundary series, in-process exchange as in test_gpu_tiles) does not take the kept tape: its recomputation runs the
    chained launch as before.  Forced staging rows, small groups, several storage chunks: bit-identical to the single domain."""
    import test_gpu_tiles as tt
    from test_gpu_parity import _run_adjoint
    g = tt._short("gr_b_64x64x720_nse", 96)
    monkeypatch.setenv("SMASHX_KEEP_CHAIN_TAPE", "1")
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", "0")
    ref = _run_adjoint(g)
    monkeypatch.setenv("SMASHX_CHAIN_STAGE", "1")
    tms = tt._check_partitioned(g, 2, 32, 32, None, reference=ref, group_size=64)
    assert any(t["chain_staged"] for t in tms.values())
    for t in tms.values():
        assert t["n_chunks"] == 3
        if t["n_chained_groups"] > 0:
            assert t["route_fwd_chained_launches"] == 2 * 3 - 1, t
