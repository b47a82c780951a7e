"""GPU: smashx_mean_forcing -- compute_mean_forcing (mw_forcing_statistic.f90:18-75) on the plan's resident forcing -- against the
arrays recorded from the compiled reference (tests/golden/mean_forcing/*.npz) and, where the reference did not go, against the fp32
numpy restatement that is pinned to those fixtures on the CPU (tests/mean_forcing_util.py, tests/test_mean_forcing_cpu.py).

Every comparison is EXACT EQUALITY OF fp32 BIT PATTERNS with NaN = NaN (a step without a value >= 0 is 0 / 0; the host's NaN carries a
sign bit the device's does not), in the default build and in the exact-libm build alike: the same IEEE additions in the same order,
one conversion, one division, no libm function involved.  There is no tolerance anywhere.

Every GPU step runs in a child process of its own (tests/mean_forcing_worker.py <step>) under a time limit of its own; the library
build is chosen per child (SMASHX_EXACT_LIBM).  The steps take a few seconds each (most of it process start and plan creation);
nothing at workload size runs here: the sizes belong to tools/mean_forcing_bench.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
LIMIT = 300
BUILDS = {"default": "0", "exact": "1"}


def _step(step, build, with_stderr=False):
    env = dict(os.environ, SMASHX_EXACT_LIBM=BUILDS[build])
    env.pop("SMASHX_MF_PIECE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "mean_forcing_worker.py"), step], env=env, capture_output=True, text=True,
                       timeout=LIMIT, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, f"step {step} ({build} build) failed with status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"OK {step} {'exact-libm' if build == 'exact' else 'default'} build" in r.stdout
    return (r.stdout, r.stderr) if with_stderr else r.stdout


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_fixture_in_every_layout_equals_the_reference(build):
    """dense, sparse and compact residency of the five recorded cases, the 0 / 0 steps of the blanked variant included (Cance and the
    blanked variant: compact requested; Cance's forcing went through float64 and PET blanked at one hour of a day is not daily x ratio,
    so both stay in fp32 rows)"""
    out = _step("fixtures", build)
    assert out.count("0 + 0 differ from the reference, 0 + 0 kept the sentinel") == 15


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_cance_in_the_compact_layout(build):
    """Cance on the reader's fp32 form loads into the compact layout: equal to the numpy restatement, and to the fp32-rows plan"""
    _step("cance_compact", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_list_in_pieces_over_several_launches(build):
    """96 x 96 x 200 with gaps, a 9216-cell list and two nested ones: SMASHX_MF_PIECE = 2048 (5 launches, the running sums carried on the
    device) equals the restatement and the default piece, in the compact layout and in fp32 rows"""
    _step("pieces", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_one_block_per_launch(build):
    """SMASHX_MF_PIECE = 64 puts a launch boundary on every block boundary: the ragged fixture (561 cells = 9 blocks, the last partly
    padding, 240 steps) equals the fixture and the default piece; a 64-cell catchment (one full block, no padding entry) equals the
    restatement; compact and fp32 rows.  Per layout the library reports 1, 9, 1 and 1 launches"""
    out, err = _step("block_pieces", build, with_stderr=True)
    assert out.count("0 + 0 differ from the reference, 0 + 0 kept the sentinel") == 8
    launches = [int(l.rsplit(",", 1)[1].split()[0]) for l in err.splitlines() if l.startswith("smashx: mean_forcing ")]
    assert launches == [1, 9, 1, 1] * 2, launches


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_one_output_alone(build):
    """mean_pet = NULL / mean_prcp = NULL: the other half equals the full call's and is fully overwritten"""
    _step("one_output", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals(build):
    """no forcing: E_STATE; NULL plan or two NULL outputs: E_ARG; 2 x 2 tiles and a catchment with an inactive cell: E_UNSUPPORTED;
    ng = 0: OK, nothing written"""
    _step("refusals", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_python_drop_in(build):
    """smash_amd.compute_mean_forcing(setup, mesh, input_data) fills input_data.mean_prcp / mean_pet in place"""
    _step("python", build)
