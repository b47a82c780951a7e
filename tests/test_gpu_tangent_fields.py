"""GPU: the tangent-linear model (smashx_forward_d: sx_tangent.h, sx_k_vert_fwd_d, the mode-2 routing pass, sx_k_cost_tangent) along
ONE FIELD at a time -- every parameter and every initial state of every structure -- held to the fp64 truth and to the adjoint sweep
of the same build.  tests/tangent_field_cases.py says why a composite direction hides the weak fields (hi, ci, cp) behind the strong
ones (hft, hlr, lr) and why the fixtures' PET is floored for the truth rule; tests/test_tangent_fields_cpu.py shows on the oracle alone
that the bars below assert something.

Per structure (one test, all fields in a loop; one plan and one adjoint sweep per case and forcing variant):
  * "floor" variant, per field: qsim_d per gauge and cost_d by the rule of tests/test_gpu_parity_at_size.py, unchanged --
    rel_l2(hip, truth64) <= 2 rel_l2(oracle32, truth64) + 1e-6, |hip - truth| <= 2 |ref - truth| + 3e-7 for cost_d.  With
    e_ref <= 1e-4 on every field this is at most 2e-4 on the weakest and about 1e-6 on most;
  * both variants, per field: the identity cost_d = <grad_f, d_f> against the gradient of the build's own adjoint sweep,
    gap_hip <= 2 gap_ref32 + 2e-5 scale (gap_ref32: the fp32 oracle's own gap along the same direction; 2e-5: the bar of
    tests/test_gpu_tangent.py::test_scalar_product; scale = sum |g_i d_i|);
  * a field the structure does not read: cost_d and qsim_d exactly zero.
Single cells of gr_c_32x32x240_d8_ragged (a direction of 1 on one cell): the same identity with scale = |g|, and cost_d and qsim_d
exactly zero wherever the oracle's gradient element is -- lr and hlr on a headwater, every field on a cell that drains to no gauge.
Storage chunks: the hft and hi directions of gr-c with chunk_steps=32, bit-identical to the single chunk.
Every (structure, field, variant) prints its lines; both builds run the same asserts (test_exact_build_runs_this_file)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bounds_cases as bc
import golden_util as gu
import tangent_field_cases as tf

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _exact_zero(t):
    return float(t["cost_d"]) == 0.0 and not np.any(np.asarray(t["qsim_d"]))


@pytest.mark.parametrize("structure", bc.STRUCTURES)
def test_every_field_direction_vs_truth_and_adjoint(structure):
    bad, worst = [], {"gap_hip": 0.0, "gap_ref32": 0.0, "e_hip": 0.0, "e_ref": 0.0}
    sweeps = {}
    for variant in tf.VARIANTS:
        for f in tf.fields(structure):
            g = tf.load(tf.case_name(structure, f), variant)
            if g.id not in sweeps:
                sweeps[g.id] = tf.Sweeps(g)
            s = sweeps[g.id]
            direction = tf.field_direction(g, f)
            d = tf.plane(direction, f)
            label = f"{structure} {variant:5s} {f:6s}"
            hip = s.tangent(direction)
            ref32 = tf.oracle_tangent(g, direction)
            b, rel = tf.identity_failures(label, hip["cost_d"], s.gradient()[f], ref32, tf.oracle_gradient(g)[f], d)
            bad += b
            worst["gap_hip"], worst["gap_ref32"] = max(worst["gap_hip"], rel[0]), max(worst["gap_ref32"], rel[1])
            if variant == "floor":
                ref64 = tf.oracle_tangent(g, direction, fp64=True)
                bad += tf.truth_failures(label, hip, ref32, ref64)
                for i in range(ref64["qsim_d"].shape[0]):
                    worst["e_hip"] = max(worst["e_hip"], gu.rel_l2(hip["qsim_d"][i], ref64["qsim_d"][i]))
                    worst["e_ref"] = max(worst["e_ref"], gu.rel_l2(ref32["qsim_d"][i], ref64["qsim_d"][i]))
        g = tf.load(tf.CASES[structure], variant)
        t = sweeps[g.id].tangent(tf.field_direction(g, tf.UNUSED[structure]))
        print(f"{structure} {variant:5s} unused {tf.UNUSED[structure]}: cost_d {t['cost_d']!r}  max |qsim_d| {np.abs(t['qsim_d']).max()!r}")
        if not _exact_zero(t):
            bad.append(f"{structure} {variant} unused {tf.UNUSED[structure]} is not zero")
    print(f"{structure}: worst gap_hip / scale {worst['gap_hip']:.2e}  gap_ref32 / scale {worst['gap_ref32']:.2e}  "
          f"worst e_hip {worst['e_hip']:.2e}  e_ref {worst['e_ref']:.2e}")
    assert not bad, bad


def test_single_cell_directions():
    g = tf.load(tf.CELL_CASE)
    h = tf.without_first_gauge(g)
    bad = []
    for case, sites in ((g, tf.cell_sites(g.mesh)), (h, {"no_gauge": tf.no_gauge_site(h.mesh)})):
        s = tf.Sweeps(case)
        grad32 = tf.oracle_gradient(case)
        for f in tf.CELL_FIELDS:
            for k, cell in sites.items():
                direction = tf.cell_direction(case, f, cell)
                label = f"cell {f:4s} {k:9s} {cell}"
                hip = s.tangent(direction)
                if float(grad32[f][cell]) == 0.0:
                    print(f"{label} oracle gradient 0: cost_d {hip['cost_d']!r}  max |qsim_d| {np.abs(hip['qsim_d']).max()!r}  "
                          f"gradient {float(s.gradient()[f][cell])!r}")
                    if not (_exact_zero(hip) and float(s.gradient()[f][cell]) == 0.0):
                        bad.append(label + " is not zero")
                else:
                    b, _ = tf.identity_failures(label, hip["cost_d"], s.gradient()[f], tf.oracle_tangent(case, direction), grad32[f],
                                                tf.plane(direction, f))
                    bad += b
    assert not bad, bad


def test_field_directions_across_storage_chunks():
    """hft (the strongest direction) and hi (the weakest, on the interception kink) of gr-c, raw forcing, cut into storage chunks of
    32 steps: cost_d, qsim_d and qsim bit-identical to the single chunk."""
    g = tf.load(tf.CASES["gr-c"], "raw")
    one, cut = tf.Sweeps(g, chunk_steps=0), tf.Sweeps(g, chunk_steps=32)
    for f in ("hft", "hi"):
        direction = tf.field_direction(g, f)
        a, b = one.tangent(direction), cut.tangent(direction)
        assert one.chunk_steps() >= g.nt and 0 < cut.chunk_steps() <= 32, (one.chunk_steps(), cut.chunk_steps())      # 1 chunk, 3 chunks
        assert a["cost_d"] == b["cost_d"] and a["cost_d"] != 0.0, (f, a["cost_d"], b["cost_d"])
        assert np.array_equal(a["qsim_d"], b["qsim_d"]) and np.array_equal(a["qsim"], b["qsim"]), f


def test_exact_build_runs_this_file():
    """the library is chosen at import time: the same cases under SMASHX_EXACT_LIBM=1 in a child process"""
    if os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0"):
        pytest.skip("already the exact-libm build: this is the child run")
    env = dict(os.environ, SMASHX_EXACT_LIBM="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "--deselect", os.path.relpath(os.path.abspath(__file__), ROOT) + "::test_exact_build_runs_this_file"], env=env,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    sys.stdout.write("".join(ln + "\n" for ln in r.stdout.splitlines() if ": worst gap_hip" in ln) + r.stdout[-3000:])
    assert r.returncode == 0 and "7 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
