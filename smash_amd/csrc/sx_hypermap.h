// sx_hypermap.h -- the hyper-linear / hyper-polynomial maps of the regionalisation on the device (include/smashx_hyper.h):
// hyper_parameters_to_parameters / hyper_states_to_states (mwd_parameters_manipulation.f90:304-362, mwd_states_manipulation.f90:270-329)
// and their adjoints HYPER_*_TO_*_B (forward_db.f90:1434-1537, 2272-2369), operation for operation what sx_hyper.cpp does on the host:
//     field_i = (ub_i - lb_i) * (1 / (1 + expf(-(h(1,i) + sum_j a_ij * d_j ** b_ij)))) + lb_i          per active cell
//     g = e * w * field_b / ((e + 1) * (e + 1)),  h_b(1,i) = sum g,  a_b = sum d ** b * g,  b_b = sum over d > 0 of d ** b * logf(d) * (a * g)
// fp32, no product contracted into an addition, expf / powf / logf as glibc evaluates them (sx_libm.h, in BOTH builds: the map runs
// once per evaluation and the mapped planes are held to the reference's bits), an exponent of exactly 1 returns the base.
//
// The descriptors lie in HBM in plan-cell order, desc[j * n + k].  The sums are sequential in the reference's order -- column index
// outer, row index inner, i.e. ascending flat index -- over the active cells only (an inactive cell carries a zero gradient: it adds
// +0 to every sum, and a sum that starts at +0 does not change by it).  So the parallelism of the adjoint is over CHAINS, one per
// (field with a slot, coefficient), and it goes in two kernels over a SPAN of cells at a time (the whole grid's terms would be
// cells x chains floats; the plan leaves no room for that):
//   sx_k_hyper_terms   the parallel part, one thread per (cell of the span, field): the linear form, e, g and the nh terms of the
//                      field's chains, stored in the staging rows terms[cell of the span][chain] -- chain-fastest
//   sx_k_hyper_walk    the ordered part, one LANE per chain, 64 chains per wavefront: down the span's rows, one addition per row.
//                      A row's load does not depend on the chain's value, so SX_HM_ROWS rows are in flight while the previous
//                      SX_HM_ROWS are added; the lanes of a wavefront read consecutive floats of a row.
// The chain values travel between the spans in sums[chain]; the host closes.  SMASHX_HYPER_SPAN in the environment forces the span
// (cells), so that a small mesh crosses several; the default keeps the staging rows at SX_HM_STAGE_BYTES.
#pragma once

#include "sx_fields.h"
#include "sx_libm.h"

#define SX_HM_ROWS 16                              // rows of the staging buffer a walking lane holds in registers
#define SX_HM_STAGE_BYTES ((size_t)32 << 20)       // staging rows of a span, default

// the fields of one launch: md_constant number (column of the hyper matrix), bounds, and where the values go / the gradient lies
struct SxHmFields {
    int nf;
    int field[SX_NFIELDS];
    float lb[SX_NFIELDS], w[SX_NFIELDS];           // lb, ub - lb
    float* val[SX_NFIELDS];                        // cell vector of the slot (or a staging vector); never null
    float* start[SX_NFIELDS];                      // the values a sweep starts from, when they are another vector (states); may be null
    float* full[SX_NFIELDS];                       // (nrow, ncol) plane the downloads read; may be null
    const float* grad[SX_NFIELDS];                 // cell gradient after an adjoint sweep (terms kernel only)
};

// d ** b the way the reference's compiler evaluates it: a call of powf, an exponent of exactly 1 returns the base
__device__ __forceinline__ float sx_hm_powb(float d, float b) { return b == 1.f ? d : sx_g_powf(d, b); }
template <bool POLY> __device__ __forceinline__ float sx_hm_a(const float* h, int j) { return POLY ? h[2 * j + 1] : h[j + 1]; }
template <bool POLY> __device__ __forceinline__ float sx_hm_b(const float* h, int j) { return POLY ? h[2 * j + 2] : 1.f; }

// h(1) + sum_j a_j d_j ** b_j at plan cell k, column h of the hyper matrix
template <bool POLY>
__device__ __forceinline__ float sx_hm_lin(const float* __restrict__ h, const float* __restrict__ desc, int nd, int n, int k) {
    float p = h[0];
    for (int j = 0; j < nd; ++j)
        p = __fadd_rn(p, __fmul_rn(sx_hm_a<POLY>(h, j), sx_hm_powb(desc[(size_t)j * n + k], sx_hm_b<POLY>(h, j))));
    return p;
}

// grid = (ceil(n / 256), F.nf), block = 256.  hyper: (nh, 24) column-major; flat: k -> row + col * nrow
template <bool POLY>
__global__ __launch_bounds__(256)
void sx_k_hyper_map(SxHmFields F, const float* __restrict__ hyper, const float* __restrict__ desc, const int* __restrict__ flat,
                    int nd, int nh, int n) {
    SX_LIBM_INIT();      // exact-libm build: the tables of expf / logf / powf into LDS (sx_libm.h); nothing otherwise
    const int k = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (k >= n) return;
    const float p = sx_hm_lin<POLY>(hyper + (size_t)F.field[e] * nh, desc, nd, n, k);
    const float v = __fadd_rn(__fmul_rn(F.w[e], 1.f / __fadd_rn(1.f, sx_g_expf(-p))), F.lb[e]);      // sigmoid, lambda = 1
    F.val[e][k] = v;
    if (F.start[e]) F.start[e][k] = v;
    if (F.full[e]) F.full[e][flat[k]] = v;
}

// grid = (ceil(ns / 256), F.nf), block = 256.  order: position among the active cells in column-major order -> plan cell; the span is
// positions [c0, c0 + ns); terms: [ns][nchain], the chains of field e of the launch are e * nh .. e * nh + nh - 1 in the hyper matrix's
// row order
template <bool POLY>
__global__ __launch_bounds__(256)
void sx_k_hyper_terms(SxHmFields F, const float* __restrict__ hyper, const float* __restrict__ desc, const int* __restrict__ order,
                      int nd, int nh, int n, int c0, int ns, float* __restrict__ terms, int nchain) {
    SX_LIBM_INIT();
    const int i = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (i >= ns) return;
    const int k = order[c0 + i];
    const float* h = hyper + (size_t)F.field[e] * nh;
    const float ex = sx_g_expf(-sx_hm_lin<POLY>(h, desc, nd, n, k));
    const float t = __fadd_rn(ex, 1.f);
    const float g = __fmul_rn(__fmul_rn(ex, F.w[e]), F.grad[e][k]) / __fmul_rn(t, t);
    float* row = terms + (size_t)i * nchain + (size_t)e * nh;
    row[0] = g;
    for (int j = 0; j < nd; ++j) {
        const float d = desc[(size_t)j * n + k];
        const float pw = sx_hm_powb(d, sx_hm_b<POLY>(h, j));
        if (POLY) {
            row[2 * j + 1] = __fmul_rn(pw, g);
            // the reference skips d <= 0; +0 leaves a sum that started at +0 as it is
            row[2 * j + 2] = d <= 0.f ? 0.f : __fmul_rn(__fmul_rn(pw, sx_g_logf(d)), __fmul_rn(sx_hm_a<POLY>(h, j), g));
        } else {
            row[j + 1] = __fmul_rn(pw, g);
        }
    }
}

// grid = ceil(nchain / 64), block = 64: lane = chain.  resume = 0: the chains start at +0, else at sums[chain]
__global__ __launch_bounds__(64)
void sx_k_hyper_walk(const float* __restrict__ terms, int ns, int nchain, float* __restrict__ sums, int resume) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nchain) return;
    float s = resume ? sums[c] : 0.f;
    const float* p = terms + c;
    float v[SX_HM_ROWS];
    int i = 0;
    if (ns >= SX_HM_ROWS) {
#pragma unroll
        for (int u = 0; u < SX_HM_ROWS; ++u) v[u] = p[(size_t)u * nchain];
    }
    for (; i + SX_HM_ROWS <= ns; i += SX_HM_ROWS) {
        const bool more = i + 2 * SX_HM_ROWS <= ns;            // uniform: every lane walks the same rows
        float nx[SX_HM_ROWS];
        if (more) {
#pragma unroll
            for (int u = 0; u < SX_HM_ROWS; ++u) nx[u] = p[(size_t)(i + SX_HM_ROWS + u) * nchain];
        }
#pragma unroll
        for (int u = 0; u < SX_HM_ROWS; ++u) s = __fadd_rn(s, v[u]);
        if (more) {
#pragma unroll
            for (int u = 0; u < SX_HM_ROWS; ++u) v[u] = nx[u];
        }
    }
    for (; i < ns; ++i) s = __fadd_rn(s, p[(size_t)i * nchain]);
    sums[c] = s;
}
