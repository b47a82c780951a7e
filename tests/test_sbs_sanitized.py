"""CPU: the library's step-by-step optimiser (smash_amd/csrc/sx_sbs.cpp: host C++, never touches the GPU) under AddressSanitizer +
UndefinedBehaviorSanitizer.  The harness tests/csrc/sx_sbs_check.cpp is a program of its own: it drives the optimiser through the C
entry points of include/smashx_sbs.h on a closed-form cost and checks the invariants (candidates in the box, batch sizes, a cost that
never rises, the evaluation count).  Nothing is preloaded and nothing is loaded into Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    exe = os.path.join(HERE, "csrc", "sx_sbs_check_asan")
    src = [os.path.join(HERE, "csrc", "sx_sbs_check.cpp"), os.path.join(ROOT, "smash_amd", "csrc", "sx_sbs.cpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in src):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", exe] + src, capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("sanitizer build unavailable: " + r.stderr[-300:])
    return exe


def _run(exe, n, seed, maxiter):
    r = subprocess.run([exe, str(n), str(seed), str(maxiter)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "VIOLATION" not in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr[-1500:])
    return r.stdout.strip()


@pytest.mark.parametrize("n,maxiter", [(1, 40), (2, 30), (3, 40), (7, 25), (24, 6)])
def test_sbs_under_address_and_ub_sanitizers(n, maxiter):
    exe = _build()
    for seed in (1, 2, 3):
        out = _run(exe, n, seed, maxiter)
        assert out.startswith(f"ok n {n} ") and ("CONVERGENCE: DDX < 0.01" in out or "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT" in out), out


def test_sbs_takes_its_branches_on_the_closed_form_cost():
    """the run of n = 3 takes line-search steps and ends by the step rule; maxiter = 0 asks for nothing"""
    exe = _build()
    out = _run(exe, 3, 1, 60)
    words = out.split()
    assert int(words[words.index("line-search") + 1]) > 0 and "CONVERGENCE: DDX < 0.01" in out, out
    out = _run(exe, 3, 1, 0)
    assert out.startswith("ok n 3 it 0 nfg 1 batches 0"), out
