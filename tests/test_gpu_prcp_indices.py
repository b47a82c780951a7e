"""GPU: smashx_prcp_indices -- compute_prcp_indices (mw_forcing_statistic.f90:77-220) on the plan's resident rain -- against the
arrays recorded from the compiled reference (tests/golden/prcp_indices/*.npz) and, where the reference did not go, against the fp32
numpy restatement that is pinned to those fixtures on the CPU (tests/prcp_indices_util.py, tests/test_prcp_indices_cpu.py).

Every comparison is EXACT EQUALITY OF fp32 BIT PATTERNS with NaN = NaN over the whole (4, ng, nt) array, prefilled with a sentinel, so
that the set of entries a call leaves alone is compared as well; in the default build and in the exact-libm build alike: the same
IEEE additions and products in the same order, IEEE divisions and square root, no libm function involved.  There is no tolerance.

Every GPU step runs in a child process of its own (tests/prcp_indices_worker.py <step>) under a time limit of its own; the library
build is chosen per child (SMASHX_EXACT_LIBM).  The steps take a few seconds each (most of it process start and plan creation);
nothing at workload size runs here: the sizes belong to tools/prcp_indices_bench.py."""
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
    env.pop("SMASHX_PI_PIECE", None)
    env.pop("SMASHX_MF_PIECE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "prcp_indices_worker.py"), step], env=env, capture_output=True, text=True,
                       timeout=LIMIT, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, f"step {step} ({build} build) failed with status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"OK {step} {'exact-libm' if build == 'exact' else 'default'} build" in r.stdout
    return (r.stdout, r.stderr) if with_stderr else r.stdout


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_fixture_in_every_layout_equals_the_reference(build):
    """dense, sparse and compact residency of the five recorded fixtures (Cance: compact requested; its rain went through float64, so
    the plan stays in fp32 rows): the bits of the reference, and the untouched set equals the fixture's"""
    out = _step("fixtures", build)
    assert out.count("(the same set: True)") == 15 and out.count(", 0 entries differ from the reference") == 15


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_lists_in_pieces_over_several_launches(build):
    """96 x 96 x 200 with gaps, the outlet's catchment plus its bins and two nested gauges: SMASHX_PI_PIECE = 4096 (5 launches, the
    sums carried on the device) equals the restatement and the default piece, in the compact layout and in fp32 rows"""
    _step("pieces", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_one_block_per_launch(build):
    """SMASHX_PI_PIECE = 64 puts a launch boundary on every block boundary, section boundaries and bin-completing blocks included: the
    ragged fixture equals the fixture, untouched set included, and the default piece, in the compact layout and in fp32 rows; the
    forced calls take one launch per block of the longest list, the others one"""
    import re
    out, err = _step("block_pieces", build, with_stderr=True)
    assert out.count("(the same set: True)") == 4 and out.count(", 0 entries differ from the reference") == 4
    runs = [(int(a), int(b)) for a, b in re.findall(r"smashx: prcp_indices .*?longest list (\d+) blocks.*?, (\d+) launches", err)]
    assert len(runs) == 4 and runs[0][0] > 9 and [b for _, b in runs] == [1, runs[0][0]] * 2, runs


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_second_flwdst_and_mean_forcing_alongside(build):
    """another flwdst plane gives that plane's result, the first one again the first; smashx_mean_forcing before, between and after
    the calls stays bit-equal to its own fixture, whichever of the two builds the catchment lists"""
    _step("second_plane", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals(build):
    """no forcing: E_STATE; a NULL plan, flwdst or output: E_ARG; 2 x 2 tiles, a one-cell catchment, a (row, row) cell that is inactive
    or outside the grid: E_UNSUPPORTED; ng = 0: OK, nothing written"""
    _step("refusals", build)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_python_drop_ins(build):
    """smash_amd.compute_prcp_indices(setup, mesh, input_data, prcp_indices) in place, smash_amd.prcp_indices(setup, mesh, input_data)"""
    _step("python", build)
