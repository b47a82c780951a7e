"""GPU: the DEVICE build of the math layer (smash_amd/csrc/sx_math.h, and sx_libm.h in the exact-libm build) against glibc, a correctly
rounded value and the host build of the same headers, over the whole float domain.

tests/test_sx_math.py proves the headers' claims on the host build (g++); the kernels run the device build, which differs exactly where
those claims live: v_rcp / v_rsq / v_sqrt seeds, ocml's fp64 exp, the wave-uniform ballot shortcuts, and the exact build's tables in LDS.
smashx_selftest_eval (include/smashx.h) evaluates one function id per element with element i on lane i % 64, so every argument set here
runs twice: as generated (sorted sweeps: wavefronts of uniform arguments, the shortcuts run) and "mixed" (one lane of every wavefront
replaced by an odd operand that forces the guarded form).  The library under test is chosen at import time (SMASHX_EXACT_LIBM=1: the
exact-libm build; tests/test_gpu_exact.py runs this module that way in its own process) and the host reference library follows it.
Counts and worst ulp distances of every check are summarised in DESIGN.md 5."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sx_host  # noqa: E402
from smash_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
EXACT = _lib.EXACT
CHUNK = 1 << 25
FP = C.POINTER(C.c_float)
(TANH, TANH_B, EXPM1, EXP, LOG, POW, POWB, M4, M4_M5, M025, M025_M125, P35, P35_25, DIV, DIV4, FDIV, DIV_FAST) = range(17)
PAIRED = (POWB, M4_M5, M025_M125, P35_25)
HOST, GLIBC, CR = "host", "glibc", "cr"
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.1754944e-38, 3.4028235e38, -3.4028235e38,
                     1.0, -1.0, 0.5, 2.0], np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(FP)


@pytest.fixture(scope="module")
def H():
    return sx_host.load(EXACT)


def device(fn, x, y=None):
    n = x.size
    o0 = np.empty(n, np.float32)
    o1 = np.empty(n, np.float32) if fn in PAIRED else None
    f = _lib.lib().smashx_selftest_eval
    _lib.check(f(0, fn, _p(x), _p(y), n, _p(o0), _p(o1)))
    return o0, o1


def reference(L, kind, fn, x, y=None):
    n = x.size
    o0 = np.empty(n, np.float32)
    o1 = np.empty(n, np.float32) if fn in PAIRED else None
    if kind == HOST:
        L.sxt_eval(fn, _p(x), _p(y), n, _p(o0), _p(o1))
    else:
        L.sxt_ref(0 if kind == GLIBC else 1, fn, _p(x), _p(y), n, _p(o0), _p(o1))
    return o0, o1


def bits(lo, hi, stride):
    """the floats with bit patterns lo, lo + stride, ... < hi, in chunks"""
    L = sx_host.load(EXACT)
    for a in range(lo, hi, CHUNK * stride):
        n = min(CHUNK, (hi - a + stride - 1) // stride)
        x = np.empty(n, np.float32)
        L.sxt_fill_bits(a, stride, n, _p(x))
        yield x


def mix(fn, x, y, odd):
    """one lane of every wavefront (lane w % 64 of wavefront w) gets the odd operand(s)"""
    unit = 4 if fn == DIV4 else 1
    nw = x.size // unit // 64
    t = np.arange(nw, dtype=np.int64) * 64 + np.arange(nw, dtype=np.int64) % 64
    el = (t[:, None] * unit + np.arange(unit)).ravel()
    x = x.copy()
    x[el] = odd[0]
    if y is not None:
        y = y.copy()
        y[el] = odd[1]
    return x, y


class Tally:
    """per check: arguments, results whose bits differ, largest ulp distance, and the first offending arguments"""

    def __init__(self, name):
        self.name, self.rows = name, {}

    def add(self, H, key, x, y, got, want):
        o, first = (C.c_longlong * 2)(), (C.c_long * 4)()
        H.sxt_compare(_p(got), _p(want), got.size, o, first, 4)
        r = self.rows.setdefault(key, {"n": 0, "mismatches": 0, "max_ulp": 0, "examples": []})
        r["n"] += got.size
        r["mismatches"] += o[0]
        r["max_ulp"] = max(r["max_ulp"], o[1])
        for i in first:
            if i >= 0 and len(r["examples"]) < 4:
                r["examples"].append((float(x[i]).hex(), None if y is None else float(y[i]).hex(), float(got[i]).hex(), float(want[i]).hex()))

    def __getitem__(self, key):
        return self.rows[key]

    def report(self):
        path = os.environ.get("SX_MATH_REPORT")
        if path:
            with open(path, "a") as f:
                f.write(json.dumps({"test": self.name, "exact": EXACT, "rows": {" ".join(map(str, k)): v for k, v in self.rows.items()}}) + "\n")
        return self


def run(H, T, fn, sets, kinds, odd=None):
    """evaluate fn on the device for every (x, y) of sets, as generated and mixed with the odd operands, against each reference kind"""
    for x, y in sets:
        refs = {k: reference(H, k, fn, x, y) for k in kinds}
        forms = [("uniform", x, y, refs)]
        if odd is not None:
            xm, ym = mix(fn, x, y, odd)
            rm = {k: reference(H, k, fn, xm, ym) for k in kinds}     # (the odd lanes' references; the rest are the same)
            forms.append(("mixed", xm, ym, rm))
        for form, xx, yy, rr in forms:
            got = device(fn, xx, yy)
            for k in kinds:
                for j in range(2 if fn in PAIRED else 1):
                    T.add(H, (fn, j, k, form), xx, yy, got[j], rr[k][j])
    return T


def clean(T, key_prefix):
    """every row whose key starts with key_prefix: zero differing bit patterns"""
    bad = {k: v for k, v in T.rows.items() if k[:len(key_prefix)] == key_prefix and v["mismatches"]}
    return not bad, bad


def _one(x):
    return [(x, None)]


# ---------------------------------------------------------------------------------------------------------------------------- tanh, expm1
def test_tanh_and_expm1_bit_identical_to_glibc(H):
    """sx_tanhf (the wave-uniform fast form and the branchy restatement) and sx_expm1f on EVERY float in +-[2^-63, 24) (1.1e9 each),
    outside that range on a stride with the special values: bit-identical to glibc's tanhf / expm1f.  The fast form runs in uniform
    wavefronts and, mixed with one |x| = 10 lane, must not."""
    T = Tally("tanh_expm1")
    for sign in (0, 0x80000000):
        for x in bits(0x20000000 + sign, 0x41C00000 + sign, 1):
            run(H, T, TANH, _one(x), [GLIBC], odd=(np.float32(10.0), None))
            run(H, T, TANH_B, _one(x), [GLIBC])
            run(H, T, EXPM1, _one(x), [GLIBC])
        for lo, hi in ((0, 0x20000000), (0x41C00000, 0x7F800001)):
            for x in bits(lo + sign, hi + sign, 97):
                for fn in (TANH, TANH_B, EXPM1):
                    run(H, T, fn, _one(x), [GLIBC], odd=(np.float32(10.0), None) if fn == TANH else None)
    for fn in (TANH, TANH_B, EXPM1):
        run(H, T, fn, _one(SPECIALS), [GLIBC])
    T.report()
    ok, bad = clean(T, ())
    assert ok, bad


# ------------------------------------------------------------------------------------------------------------------------ the fixed powers
FIXED = (M4, M4_M5, M025, M025_M125, P35, P35_25)
FIXED_SPECIALS = np.array([0.0, np.inf, np.nan, 1e-45, 1e-40, 1.1754942e-38, 1.1754944e-38, 3.4028235e38, 1.0, 2.0**-32, 2.0**32],
                          np.float32)


def test_fixed_powers(H):
    """x^-4, x^-5, y^-1/4, y^-5/4, h^3.5, h^2.5, single and paired.  Default build, on its domain (positive normal arguments,
    sx_math.h): within 1 ulp of the correctly rounded power on every 13th float, and equal to the host build of the header except in
    at most 1e-6 of the arguments, by one ulp (the hardware seed's last bits reach the result in ~1e-7); subnormals, 0, inf and NaN are
    measured and reported.  Exact build: bit-identical to glibc powf (every 11th base in [1e-7, 1e4] as on the host, every 1009th
    float of the whole range, the special values)."""
    T = Tally("fixed_powers")
    if not EXACT:
        Tout = Tally("fixed_powers_outside_domain")
        for x in bits(0x00800000, 0x7F800000, 13):
            for fn in FIXED:
                run(H, T, fn, _one(x), [HOST, CR], odd=(np.float32(1.0), None))
        for x in bits(0, 0x00800000, 13):
            for fn in FIXED:
                run(H, Tout, fn, [(np.concatenate([x, FIXED_SPECIALS]), None)], [HOST, CR])
        T.report()
        Tout.report()
        for k, r in T.rows.items():
            if k[2] == CR:
                assert r["max_ulp"] <= 1, (k, r)
            else:
                assert r["max_ulp"] <= 1 and r["mismatches"] <= 1e-6 * r["n"], (k, r)
    else:
        odd = (np.float32(1e-40), None)      # a subnormal lane: the exact build's paired form leaves its straight path
        for lo, hi, stride in ((0x33D6BF95, 0x461C4000, 11), (0, 0x7F800001, 1009)):
            for x in bits(lo, hi, stride):
                for fn in FIXED:
                    run(H, T, fn, _one(x), [GLIBC], odd=odd)
        for fn in FIXED:
            run(H, T, fn, _one(FIXED_SPECIALS), [GLIBC])
        ok, bad = clean(T.report(), ())
        assert ok, bad


# --------------------------------------------------------------------------------------------------------------------------------- expf
def test_expf(H):
    """sx_expf on every 7th float, both signs (6.1e8).  Default build (ocml's fp64 exp, rounded once): within 1 ulp of the correctly
    rounded value, differing from it in at most 1e-7 of the arguments -- the header's claim.  Exact build: glibc's bits."""
    T = Tally("expf")
    for sign in (0, 0x80000000):
        for x in bits(sign, 0x7F800001 + sign, 7):
            run(H, T, EXP, _one(x), [CR] if not EXACT else [GLIBC], odd=(np.float32(0.0), None))
    run(H, T, EXP, _one(SPECIALS), [CR, GLIBC])
    T.report()
    if EXACT:
        ok, bad = clean(T, ())
        assert ok, bad
    else:
        for k, r in T.rows.items():
            if k[2] == CR:
                assert r["max_ulp"] <= 1 and r["mismatches"] <= 1e-7 * r["n"], (k, r)
        assert T[(EXP, 0, GLIBC, "uniform")]["max_ulp"] <= 1


# ------------------------------------------------------------------------------------------------------------------- logf, powf, powbase
def _pairs(seed, n):
    """n (x, y) pairs: the vic-a kind (bases in (0, 1) and around 1, exponents of moderate size) and arbitrary bit patterns"""
    g = np.random.default_rng(seed)
    out = []
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        q = m // 4
        x = np.concatenate([g.uniform(1e-7, 1.0, q).astype(np.float32), g.uniform(1e-3, 50.0, q).astype(np.float32),
                            (1.0 + g.uniform(-0.06, 0.06, q)).astype(np.float32),
                            g.integers(0, 2**32, m - 3 * q, dtype=np.uint64).astype(np.uint32).view(np.float32)])
        y = np.concatenate([g.uniform(0.05, 3.0, q).astype(np.float32), g.uniform(-5, 5, q).astype(np.float32),
                            g.uniform(-3, 3, q).astype(np.float32),
                            g.integers(0, 2**32, m - 3 * q, dtype=np.uint64).astype(np.uint32).view(np.float32)])
        out.append((x, y))
    return out


def _pow_specials():
    xs = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 1e-45, 1e-40, -1e-40, 3.4e38, 0.5, -0.5, np.inf, -np.inf, np.nan], np.float32)
    ys = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 3.0, -3.0, -2.5, 30.0, -30.0, 1e30, -1e30, np.inf, -np.inf, np.nan], np.float32)
    return np.repeat(xs, ys.size), np.tile(ys, xs.size)


def test_logf_powf_powbase(H):
    """sx_logf on every 5th positive float (and the negative / special ones on a stride); sx_powf and sx_powbase + sx_powb / sx_logb on
    5e7 random pairs incl. arbitrary bit patterns and on the special values of sxt_g_specials.  Default build: bit-identical to the host
    build of the header.  Exact build: bit-identical to glibc's logf / powf."""
    T = Tally("log_pow")
    kind = GLIBC if EXACT else HOST
    odd = (np.float32(0.0), np.float32(1.5))      # a zero base: the ballot shortcut of sx_log2_d / sx_pow_from must not run
    for x in bits(0, 0x7F800001, 5):
        run(H, T, LOG, _one(x), [kind], odd=odd)
    for x in bits(0x80000000, 0xFFFFFFFF, 4099):
        run(H, T, LOG, _one(x), [kind])
    run(H, T, LOG, _one(SPECIALS), [kind])
    sets = _pairs(2026, 50_000_000) + [_pow_specials()]
    run(H, T, POW, sets, [kind], odd=odd)
    run(H, T, POWB, sets, [kind], odd=odd)
    T.report()
    ok, bad = clean(T, ())
    assert ok, bad


# ------------------------------------------------------------------------------------------------------------------------------ division
def _normal_pairs(seed, n):
    """n (a, d) in the range Markstein's theorem covers: |a| in [2^-100, 2^128), |d| in [2^-125, 2^126) (1/d normal), quotient exponent
    within [-100, 100] (the residual a - d q does not underflow); every 256th d has an all-ones significand (the theorem's corner)"""
    g = np.random.default_rng(seed)
    out = []
    for a0 in range(0, n, CHUNK):
        m = min(CHUNK, n - a0)
        ed = np.repeat(g.integers(2, 253, m // 4), 4)           # one denominator per quadruple (sx_div4 divides by y[4i])
        ea = np.clip(ed + g.integers(-100, 101, m), 27, 254)
        sa = g.integers(0, 2, m, dtype=np.uint32) << 31
        sd = g.integers(0, 2, m, dtype=np.uint32) << 31
        ma = g.integers(0, 1 << 23, m, dtype=np.uint32)
        md = np.repeat(g.integers(0, 1 << 23, m // 4, dtype=np.uint32), 4)
        md[::256] = (1 << 23) - 1
        sd = np.repeat(sd[::4], 4)
        a = (sa | (ea.astype(np.uint32) << 23) | ma).view(np.float32)
        d = (sd | (ed.astype(np.uint32) << 23) | md).view(np.float32)
        out.append((a, d))
    return out


def _whole_range_pairs(seed, n):
    """arbitrary bit patterns for a and d, then the edges: subnormal numerators and results, |d| >= 2^126, subnormal d, 0, inf, NaN"""
    g = np.random.default_rng(seed)
    m = n // 4
    u = lambda k: g.integers(0, 2**32, k, dtype=np.uint64).astype(np.uint32)     # noqa: E731
    sub = lambda k: (u(k) & np.uint32(0x807FFFFF)).view(np.float32)                # noqa: E731  (subnormal or zero)
    big = lambda k: ((u(k) & np.uint32(0x807FFFFF)) | (np.uint32(253) + (u(k) & np.uint32(1))) << 23).view(np.float32)   # noqa: E731
    norm = lambda k, lo, hi: ((u(k) & np.uint32(0x807FFFFF)) | g.integers(lo, hi, k).astype(np.uint32) << 23).view(np.float32)  # noqa: E731
    a = np.concatenate([u(m).view(np.float32), sub(m), norm(m, 100, 255), norm(n - 3 * m, 1, 60)])
    d = np.concatenate([u(m).view(np.float32), norm(m, 60, 194), big(m), sub(n - 3 * m)])
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -3.0, 1e-45, 2.0**127, 2.0**-149 * 3], np.float32)
    a = np.concatenate([a, np.repeat(sp, sp.size)])
    d = np.concatenate([d, np.tile(sp, sp.size)])
    k = a.size - a.size % 4
    return [(a[:k], d[:k])]


# a huge quotient: the exact build's wave-uniform guard must take the lane (the default build has no guard: an ordinary pair there)
DIV_ODD = (np.float32(1e30), np.float32(1e-30)) if EXACT else (np.float32(3.0), np.float32(7.0))


def test_division(H):
    """sx_div (sx_mkdiv), sx_div4 (four numerators, one denominator), sx_fdiv and sx_div with sx_mkdiv_fast.
    Default build: sx_div / sx_div4 give RN(a/d) for every normal a, d with a normal quotient (Markstein); sx_fdiv / sx_mkdiv_fast are
    within 1 ulp and differ in fewer than 1e-6 of those pairs; the whole-range behaviour is reported.  Exact build: all four are the
    IEEE quotient, bit for bit, on the whole float range."""
    Tn, Tw = Tally("division_normal"), Tally("division_whole_range")
    normal = _normal_pairs(7, 40_000_000)     # (a multiple of 4)
    whole = _whole_range_pairs(8, 20_000_000)
    for fn in (DIV, DIV4, FDIV, DIV_FAST):
        run(H, Tn, fn, normal, [GLIBC], odd=DIV_ODD)
        for x, y in whole:     # (sx_div4 divides by y[4i]: every quadruple shares its first denominator)
            run(H, Tw, fn, [(x, np.repeat(y[::4], 4) if fn == DIV4 else y)], [GLIBC], odd=DIV_ODD)
    Tn.report()
    Tw.report()
    for k, r in Tn.rows.items():
        if EXACT or k[0] in (DIV, DIV4):
            assert r["mismatches"] == 0, (k, r)
        else:
            assert r["max_ulp"] <= 1 and r["mismatches"] < 1e-6 * r["n"], (k, r)
    if EXACT:
        ok, bad = clean(Tw, ())
        assert ok, bad
