"""CPU: the host side of the hyper maps on the device that is plain C++ (smash_amd/csrc/sx_hyperhost.h: argument checks, descriptor
gather, the order of the sums, closing of the gradient matrices, scatter into the caller's planes) in a stand-alone program
(tests/csrc/sx_hyperhost_check.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer, every buffer a heap block of exactly the
size a caller owes.  The device side cannot run under a sanitizer on the pool; tests/test_gpu_hyper_device.py covers its results."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "csrc", "sx_hyperhost_check")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(HERE, "csrc", "sx_hyperhost_check.cpp")
    deps = [src] + [os.path.join(HERE, "..", "smash_amd", "csrc", f) for f in ("sx_hyperhost.h", "sx_fields.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return EXE


@pytest.mark.parametrize("nrow,ncol,nd", [(33, 29, 6), (16, 16, 2), (7, 5, 0), (1, 1, 1)])
def test_host_side_under_sanitizers(exe, nrow, ncol, nd):
    r = subprocess.run([exe, str(nrow), str(ncol), str(nd)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-1500:])
