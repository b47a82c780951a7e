// sx_selftest.h -- one element of smashx_selftest_eval (include/smashx.h): the math entry `fn` of sx_math.h applied to x[i] (and y[i]).
// The device kernel (smashx.hip) and the host build of the tests (tests/csrc/sx_math_host.cpp) call this same function, so the two
// builds of the header are compared through identical wiring.  SMASHX_FN_DIV4 handles four consecutive elements 4i .. 4i+3, one
// denominator y[4i]; every other id handles element i.
#pragma once

#include "../../include/smashx.h"
#include "sx_math.h"

SX_HD void sx_selftest_eval1(int fn, const float* x, const float* y, long long i, float* o0, float* o1) {
    switch (fn) {
    case SMASHX_FN_TANH: o0[i] = sx_tanhf(x[i], true); break;
    case SMASHX_FN_TANH_BRANCHY: o0[i] = sx_tanhf(x[i], false); break;
    case SMASHX_FN_EXPM1: o0[i] = sx_expm1f(x[i]); break;
    case SMASHX_FN_EXP: o0[i] = sx_expf(x[i]); break;
    case SMASHX_FN_LOG: o0[i] = sx_logf(x[i]); break;
    case SMASHX_FN_POW: o0[i] = sx_powf(x[i], y[i]); break;
    case SMASHX_FN_POWB: { const SxPowBase B = sx_powbase(x[i]); o0[i] = sx_powb(B, y[i]); o1[i] = sx_logb(B); break; }
    case SMASHX_FN_POW_M4: o0[i] = sx_pow_m4(x[i]); break;
    case SMASHX_FN_POW_M4_M5: sx_pow_m4_m5(x[i], &o0[i], &o1[i]); break;
    case SMASHX_FN_POW_M025: o0[i] = sx_pow_m025(x[i]); break;
    case SMASHX_FN_POW_M025_M125: sx_pow_m025_m125(x[i], &o0[i], &o1[i]); break;
    case SMASHX_FN_POW_3P5: o0[i] = sx_pow_3p5(x[i]); break;
    case SMASHX_FN_POW_3P5_2P5: sx_pow_3p5_2p5(x[i], &o0[i], &o1[i]); break;
    case SMASHX_FN_DIV: o0[i] = sx_div(x[i], sx_mkdiv(y[i])); break;
    case SMASHX_FN_DIV4: {
        const float a[4] = {x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
        float q[4];
        sx_div4(q, a, sx_mkdiv(y[4 * i]));
        for (int j = 0; j < 4; ++j) o0[4 * i + j] = q[j];
        break;
    }
    case SMASHX_FN_FDIV: o0[i] = sx_fdiv(x[i], y[i]); break;
    case SMASHX_FN_DIV_FAST: o0[i] = sx_div(x[i], sx_mkdiv_fast(y[i])); break;
    default: break;
    }
}
