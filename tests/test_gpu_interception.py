"""GPU: smashx_adjust_interception -- adjust_interception_store (mw_interception_store.f90:19-160) on the plan's resident forcing --
against the planes recorded from the compiled reference (tests/golden/interception/*.npz) and, where the reference cannot go, against
the fp32 numpy restatement that is pinned to those fixtures on the CPU (tests/interception_util.py, tests/test_interception_cpu.py).

Every comparison is EXACT EQUALITY OF fp32 BIT PATTERNS, in the default build and in the exact-libm build alike: same IEEE operations in
the same order, a discrete result, no libm function involved.

Every GPU step runs in a child process of its own (tests/interception_worker.py <step>) under a time limit of its own; the library
build is chosen per child (SMASHX_EXACT_LIBM).  Limits of the small steps: 300 s each (they take a few seconds; most of it is process
start and plan creation).

The step at size -- 1024^2 cells x 8760 steps, gr-b, compact forcing built on the device block by block as bench.py builds it, 4096
randomly drawn cells against the numpy restatement on their gathered forcing columns -- measured on an MI355X (first run):
    set-up (mesh, plan, forcing) 2.4 s, smashx_adjust_interception 0.263 s wall, numpy restatement of the 4096 columns 3.5 s,
    the whole child about 10 s (all eleven children of this file together: 32 s)
Its limit is AT_SIZE_LIMIT = 120 s: twelve times the measured child, because nearly all of it is host work (mesh, schedule, numpy) whose
speed depends on the machine's CPUs and on who shares them, not on the GPU; the library call itself is bounded inside the library (the
cells go in pieces of 2^19 per launch, 0.13 s per launch at the measured rate)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
SMALL_LIMIT = 300
AT_SIZE_LIMIT = 120
BUILDS = {"default": "0", "exact": "1"}


def _step(step, build, limit, *args):
    env = dict(os.environ, SMASHX_EXACT_LIBM=BUILDS[build])
    r = subprocess.run([sys.executable, os.path.join(HERE, "interception_worker.py"), step] + [str(a) for a in args],
                       env=env, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, f"step {step} ({build} build) failed with status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"OK {step} {'exact-libm' if build == 'exact' else 'default'} build" in r.stdout
    return r.stdout


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_fixture_in_every_layout_equals_the_reference(build):
    """dense, sparse and compact residency (Cance: compact requested; its fixture forcing went through float64 and stays in fp32 rows)
    of every recorded case: the ci plane is the reference's on active cells, inactive cells keep the sentinel written beforehand"""
    out = _step("fixtures", build, SMALL_LIMIT)
    assert out.count("0 differ from the reference, 0 inactive cells lost the sentinel") == 12


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_cance_in_the_compact_layout(build):
    """Cance on the reader's fp32 form loads into the compact layout: equal to the numpy restatement, and to the fp32-rows plan"""
    _step("cance_compact", build, SMALL_LIMIT)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_two_by_two_tiling_overlays_to_the_single_domain(build):
    _step("tiles", build, SMALL_LIMIT)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals(build):
    """gr-a / gr-d / vic-a: E_UNSUPPORTED; a plan without forcing: E_STATE; NULL pointers and malformed day_index: E_ARG"""
    _step("refusals", build, SMALL_LIMIT)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_forward_with_the_adjusted_plane(build):
    """the plane goes where ci goes: a forward run after adjust_interception_store equals one with the fixture's plane put in by hand"""
    _step("forward", build, SMALL_LIMIT)


def test_at_size_against_the_numpy_restatement():
    """1024^2 x 8760, compact forcing built on the device, 4096 sampled cells (figures and the limit: module docstring)"""
    _step("at_size", "default", AT_SIZE_LIMIT, 1024, 8760, 4096)
