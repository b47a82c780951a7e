"""CPU: the host side of the ANN regionalisation that is plain C++ (smash_amd/csrc/sx_annhost.h over sx_ann.h: the graph's checks and
normal form, the device limits, the network's forward pass and weight gradient in the stated order) in a stand-alone program
(tests/csrc/sx_annhost_check.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer, every buffer a heap block of exactly the
size a caller owes.  The device side does not run under a sanitizer on a GPU; tests/test_gpu_ann.py covers its results."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "csrc", "sx_annhost_check")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(HERE, "csrc", "sx_annhost_check.cpp")
    deps = [src] + [os.path.join(HERE, "..", "smash_amd", "csrc", f) for f in ("sx_annhost.h", "sx_ann.h", "sx_hyperhost.h", "sx_fields.h")]
    deps.append(os.path.join(HERE, "..", "include", "smashx_ann.h"))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", EXE, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return EXE


@pytest.mark.parametrize("nrow,ncol,nd", [(33, 29, 6), (16, 16, 2), (1, 1, 1)])
def test_host_side_under_sanitizers(exe, nrow, ncol, nd):
    r = subprocess.run([exe, str(nrow), str(ncol), str(nd)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-1500:])
    assert int(r.stdout.split()[1]) >= 1
