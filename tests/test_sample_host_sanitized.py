"""CPU: the host side of the two sample paths that is plain C++ (smash_amd/csrc/sx_samplehost.h: the field map, the staging of a batch of
the sample -- the one place where smashx_multiple_run / smashx_uniform_costs read caller memory at a computed offset -- and the batch /
time-chunk choice) in a stand-alone program (tests/csrc/sx_samplehost_check.cpp) built with AddressSanitizer +
UndefinedBehaviorSanitizer, every buffer a heap block of exactly the size a caller owes.  The device side runs under no sanitizer;
tests/test_gpu_ensemble.py and tests/test_gpu_uniform_costs.py cover its results."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "csrc", "sx_samplehost_check")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(HERE, "csrc", "sx_samplehost_check.cpp")
    deps = [src] + [os.path.join(HERE, "..", "smash_amd", "csrc", f) for f in ("sx_samplehost.h", "sx_fields.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return EXE


@pytest.mark.parametrize("nfields", [0, 1, 3])
@pytest.mark.parametrize("nsamples,SP", [(1, 64), (63, 64), (64, 64), (65, 64), (130, 128), (130, 64)])
def test_host_side_under_sanitizers(exe, nfields, nsamples, SP):
    r = subprocess.run([exe, str(nfields), str(nsamples), str(SP)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert r.stdout == f"ok {(nsamples + SP - 1) // SP}\n" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-1500:])
