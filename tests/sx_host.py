"""The host build of smash_amd/csrc/sx_math.h (+ sx_libm.h) used by tests/test_sx_math.py and tests/test_gpu_math.py:
tests/csrc/sx_math_host.cpp compiled by g++ once per build flavour -- the default build, and -DSX_EXACT_LIBM=1 (the headers as the
libsmashx_exact.so kernels compile them).  Rebuilt when a source is newer; written to a temporary name and renamed, so two test
processes never load a half-written library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "smash_amd", "csrc")
SOURCES = [os.path.join(HERE, "csrc", "sx_math_host.cpp"), os.path.join(CSRC, "sx_math.h"), os.path.join(CSRC, "sx_libm.h"),
           os.path.join(CSRC, "sx_selftest.h"), os.path.join(HERE, "..", "include", "smashx.h")]

_cache = {}


def load(exact=False):
    if exact in _cache:
        return _cache[exact]
    so = os.path.join(HERE, "csrc", "sx_math_host_exact.so" if exact else "sx_math_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in SOURCES):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fopenmp", "-fPIC", "-shared"]
                              + (["-DSX_EXACT_LIBM=1"] if exact else []) + ["-o", tmp, SOURCES[0], "-lm"])
        os.replace(tmp, so)
    L = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    L.sxt_eval.argtypes = [C.c_int, fp, fp, C.c_long, fp, fp]
    L.sxt_ref.argtypes = [C.c_int, C.c_int, fp, fp, C.c_long, fp, fp]
    L.sxt_compare.argtypes = [fp, fp, C.c_long, C.POINTER(C.c_longlong), C.POINTER(C.c_long), C.c_int]
    L.sxt_fill_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_long, fp]
    L.sxt_div_big_denominator_mismatches.restype = C.c_long
    L.sxt_div_big_denominator_mismatches.argtypes = [C.c_long, C.c_uint]
    _cache[exact] = L
    return L
