"""CPU: the conditions under which tests/test_gpu_tangent_fields.py and the lone-field sweeps of tests/test_gpu_bounds.py assert
anything, shown on the plain-C oracle alone (tests/tangent_field_cases.py; nothing here runs a kernel).

  (a) "floor" variant (every exactly zero PET value at 0.013): along every field of every structure the fp32 oracle's qsim_d is within
      1e-4 (rel-L2, per gauge) of the fp64 truth, so the truth rule e_hip <= 2 e_ref + 1e-6 is a bar of at most 2e-4 on the weakest
      field and about 1e-6 on most.  A gauge whose fp64 qsim_d is identically zero is printed and skipped, at most one (field, gauge)
      pair per structure.
  (b) "raw" variant: along ci and along hi of gr-b and gr-c the same quantity exceeds 1e-2 on every gauge -- the interception kink at
      PET = 0, the reason the floor exists.
  (c) the fp32 oracle's own adjoint-tangent gap |cost_d - <grad_f, d_f>| is within 2e-4 of sum |g_i d_i| for every field in both
      variants (measured: 1.2e-4 at worst, cp of gr-d; mostly below 1e-5), and within 1e-12 in fp64: the helper's directions, planes
      and sums are the right ones.
  (d) over the 92 single-field cases B:<structure>:<field>:<side> of tests/bounds_cases.py, the lone-field e_ref exceeds 1e-4 on at
      most 16 (13 counted: the ci and hi cases of gr-b and gr-c, B:vic-a:b:*, B:gr-c:cst:lb, B:gr-a:cp:ub, B:gr-d:cp:ub); those take
      the identity only on the GPU -- and the ci and hi cases the truth rule on a floor copy, where e_ref is back below 1e-4.
  (e) single cells of gr_c_32x32x240_d8_ragged: the oracle's gradient element is exactly zero for lr and hlr on the two headwaters
      and for every field on the cell that drains to no gauge, nowhere else, and the oracle's tangent is exactly zero exactly there."""
import numpy as np
import pytest

import bounds_cases as bc
import tangent_field_cases as tf

_runs = {}


def _run(structure, variant):
    """field -> (direction plane, fp32 tangent, fp64 tangent, fp32 gradient plane, fp64 gradient plane), computed once."""
    if (structure, variant) not in _runs:
        out = {}
        for f in tf.fields(structure):
            g = tf.load(tf.case_name(structure, f), variant)
            d = tf.field_direction(g, f)
            out[f] = (tf.plane(d, f), tf.oracle_tangent(g, d), tf.oracle_tangent(g, d, fp64=True), tf.oracle_gradient(g)[f],
                      tf.oracle_gradient(g, fp64=True)[f])
        _runs[structure, variant] = out
    return _runs[structure, variant]


@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_floor_variant_fp32_oracle_is_near_the_truth_on_every_field(structure):
    bad, skipped = [], []
    for f, (d, r32, r64, _, _) in _run(structure, "floor").items():
        assert np.count_nonzero(d) > 0, f
        for i, e in enumerate(tf.e_ref(r32, r64)):
            if not np.any(r64["qsim_d"][i]):
                print(f"{structure} {f} gauge {i}: qsim_d is identically zero in fp64, skipped")
                skipped.append((f, i))
                continue
            print(f"{structure} floor {f:6s} gauge {i}  e_ref {e:.2e}  |qsim_d| {np.linalg.norm(r64['qsim_d'][i]):.2e}")
            if not e <= tf.E_REF_CAP:
                bad.append((f, i, e))
    assert not bad, bad
    assert len(skipped) <= 1, skipped


@pytest.mark.parametrize("structure", ["gr-b", "gr-c"])
def test_raw_variant_interception_kink_puts_fp32_far_from_the_truth(structure):
    for f in ("ci", "hi"):
        _, r32, r64, _, _ = _run(structure, "raw")[f]
        e = tf.e_ref(r32, r64)
        print(f"{structure} raw {f}: e_ref per gauge {['%.2e' % x for x in e]}")
        assert min(e) > 1e-2, (f, e)


@pytest.mark.parametrize("variant", tf.VARIANTS)
@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_oracle_identity_gap(structure, variant):
    bad = []
    for f, (d, r32, r64, g32, g64) in _run(structure, variant).items():
        sc = tf.scale(g32, d)
        gap32, gap64 = tf.gap(r32["cost_d"], g32, d), tf.gap(r64["cost_d"], g64, d)
        print(f"{structure} {variant:5s} {f:6s} gap32 / scale {gap32 / sc:.2e}  gap64 / scale {gap64 / tf.scale(g64, d):.2e}  scale {sc:.2e}")
        assert sc > 0, f
        if not (gap32 <= 2e-4 * sc and gap64 <= 1e-12 * tf.scale(g64, d)):
            bad.append((f, gap32 / sc, gap64))
        assert tf.identity_ok(gap32, gap32, sc)          # the reference alone meets the GPU's bar by construction
    assert not bad, bad


def test_unused_field_has_a_zero_tangent():
    for s, f in tf.UNUSED.items():
        assert f not in tf.fields(s)
        g = tf.load(tf.CASES[s], "raw")
        for fp64 in (False, True):
            r = tf.oracle_tangent(g, tf.field_direction(g, f), fp64=fp64)
            assert r["cost_d"] == 0.0 and not np.any(r["qsim_d"]), (s, f, fp64)


def test_floor_touches_the_zeros_of_pet_only():
    for s, name in tf.CASES.items():
        raw, fl = tf.load(name, "raw"), tf.load(name, "floor")
        zero = raw.pet == 0
        assert zero.any() and np.array_equal(fl.pet[~zero], raw.pet[~zero]) and np.all(fl.pet[zero] == tf.PET_FLOOR), s
        assert fl.pet.dtype == np.float32 and fl.prcp is not raw.prcp and np.array_equal(fl.prcp, raw.prcp), s
        assert np.array_equal(raw.pet < 0, fl.pet < 0), s          # the data gaps stay


def lone_field_e_ref(cid):
    """max over the gauges of rel_l2(oracle32 qsim_d, truth64 qsim_d) along tf.field_direction of the field on the bound."""
    g = bc.build(cid)
    d = tf.field_direction(g, cid.split(":")[2])
    return max(tf.e_ref(tf.oracle_tangent(g, d), tf.oracle_tangent(g, d, fp64=True)))


def test_bounds_cases_with_a_loose_lone_field_bar_are_few():
    single = [cid for cid in bc.ids() if cid.startswith("B:")]
    assert len(single) == 92
    loose = {cid: e for cid in single for e in [lone_field_e_ref(cid)] if not e <= tf.E_REF_CAP}
    for cid, e in loose.items():
        print(f"{cid:20s} lone-field e_ref {e:.2e}")
    assert len(loose) <= 16, loose
    for s in ("gr-b", "gr-c"):                              # and the floor brings the interception cases back
        for f in ("ci", "hi"):
            for end in ("lb", "ub"):
                g = bc.floor_copy(bc.build(f"B:{s}:{f}:{end}"))
                d = tf.field_direction(g, f)
                e = tf.e_ref(tf.oracle_tangent(g, d), tf.oracle_tangent(g, d, fp64=True))
                print(f"B:{s}:{f}:{end} floor copy: lone-field e_ref {max(e):.2e}")
                assert max(e) <= tf.E_REF_CAP, (s, f, end, e)


def test_single_cells_zero_gradient_means_zero_tangent():
    g = tf.load(tf.CELL_CASE)
    sites = tf.cell_sites(g.mesh)
    h = tf.without_first_gauge(g)
    acc = np.asarray(g.mesh.flwacc)
    assert acc[sites["first"]] == 1 and acc[sites["last"]] == 1          # headwaters: the routing reads neither lr nor hlr there
    assert tf.drains_to_a_gauge(g.mesh, tf.no_gauge_site(h.mesh)) and sites["gauge"] == tuple(np.asarray(h.mesh.gauge_pos)[0])
    assert all(tf.drains_to_a_gauge(g.mesh, c) for c in tf.active_cells(g.mesh))          # the first gauge is the outlet of the mesh
    zero = set()
    for case, ss in ((g, sites), (h, {"no_gauge": tf.no_gauge_site(h.mesh)})):
        grad = tf.oracle_gradient(case)
        for f in tf.CELL_FIELDS:
            for k, c in ss.items():
                r = tf.oracle_tangent(case, tf.cell_direction(case, f, c))
                gv = float(grad[f][c])
                print(f"{f:4s} {k:9s} {c}  g {gv: .3e}  cost_d {r['cost_d']: .3e}  gap / |g| {abs(r['cost_d'] - gv) / abs(gv) if gv else 0.0:.2e}")
                if gv == 0.0:
                    zero.add((f, k))
                    assert r["cost_d"] == 0.0 and not np.any(r["qsim_d"]), (f, k)
                else:
                    assert r["cost_d"] != 0.0 and np.any(r["qsim_d"]), (f, k)
    assert zero == {(f, k) for f in ("lr", "hlr") for k in ("first", "last")} | {(f, "no_gauge") for f in tf.CELL_FIELDS}, zero
