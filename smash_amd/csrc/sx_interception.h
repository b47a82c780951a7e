// sx_interception.h -- mw_interception_store::adjust_interception_store (smash/solver/routine/mw_interception_store.f90:19-160) on the
// forcing the plan holds in HBM: for every cell, the interception capacity out of the candidates
//     cmax(i) = stt + (i - 1) * step,  i = 1 .. ceiling((stp - stt) / step),  stt = 0.1, stp = 5, step = 0.1   (49 in fp32)
// whose interception evaporation, summed over the period step by step, comes closest to the evaporation formed from daily totals:
//     daily_cumulated = sum over days of min(sum of prcp over the day, sum of pet over the day)
//     sum(i)          = sum over steps of ec, (pth, ec) = gr_interception(prcp, pet, cmax(i), h) from h = 0
//     ci              = cmax(minloc(|sum - daily_cumulated|)), the first minimum
// all in fp32, in time order, without contraction.  The routine knows no gaps: a -99 marker goes through the arithmetic.
//
// The result is a discrete choice and exact ties between neighbouring candidates occur, so every operation must give the reference's
// bits.  The interception step is therefore restated here with the IEEE quotient in BOTH builds (sx_interception of sx_ops.h divides
// through sx_div, which is the quotient only on the range it was proven for); no libm function is involved.
//
// Mapping: a workgroup is 64 cells x SX_ICI_ROWS wavefronts; wavefront y carries SX_ICI_PER candidates (y * 7 .. y * 7 + 6) of its 64
// cells through the whole period: 7 levels + 7 sums + the day's totals in registers (8 waves per SIMD), no state in HBM, nothing
// written but the result.  The seven wavefronts of a workgroup read the same forcing words within a few steps of each other: HBM
// sees each word once, the others are cache hits.  The daily reference is two additions per step and is kept by every wavefront for
// itself.  At the end the wavefronts' best candidates meet in LDS and row 0 takes the first minimum in candidate order.
#pragma once

#include "sx_kernels.h"

#define SX_ICI_PER 7          // candidates per thread
#define SX_ICI_ROWS_MAX 8     // wavefronts per workgroup the LDS arrays are sized for (49 candidates: 7)

// the reference's candidate list: its length (the dimension expression of cmax) and its entries (arange_r, m_array_creation.f90:41-54)
#define SX_ICI_STT 0.1f
#define SX_ICI_STP 5.f
#define SX_ICI_STEP 0.1f
static inline int sx_ici_ncand() { return (int)ceilf((SX_ICI_STP - SX_ICI_STT) / SX_ICI_STEP); }
__host__ __device__ __forceinline__ float sx_ici_cmax(int i0) { return SX_ICI_STT + (float)i0 * SX_ICI_STEP; }   // i0 = i - 1

// gr_interception (md_gr_operator.f90:20-34) with the IEEE division
__device__ __forceinline__ void sx_interception_ieee(float prcp, float pet, float ci, float& hi, float& ei) {
    ei = fminf(pet, prcp + hi * ci);
    const float pn = fmaxf(0.f, prcp - ci * (1.f - hi) - ei);
    hi = hi + (prcp - ei - pn) / ci;
}

// cells [A.k0, A.k1) of the plan's order; day_index[nt]: the caller's, checked on the host (non-decreasing in steps of 0 / 1);
// ci_out[k]: the chosen capacity.  blockDim = (64, rows), rows * SX_ICI_PER >= nc.
__global__ __launch_bounds__(64 * SX_ICI_ROWS_MAX)
void sx_k_adjust_interception(SxDeviceArrays A, const int* __restrict__ day_index, int nc, float* __restrict__ ci_out) {
    __shared__ float s_diff[SX_ICI_ROWS_MAX][64];
    __shared__ int s_idx[SX_ICI_ROWS_MAX][64];
    const int k = A.k0 + blockIdx.x * 64 + threadIdx.x;
    const bool live = k < A.k1;
    const unsigned kb = (unsigned)(live ? k : A.k0) * 4u;      // lanes past the range read the first cell's forcing and store nothing
    const int c0 = threadIdx.y * SX_ICI_PER;

    float cmax[SX_ICI_PER], h[SX_ICI_PER], sum[SX_ICI_PER];
#pragma unroll
    for (int j = 0; j < SX_ICI_PER; ++j) { cmax[j] = sx_ici_cmax(c0 + j); h[j] = 0.f; sum[j] = 0.f; }

    float day_p = 0.f, day_e = 0.f, daily = 0.f;
    float pn_, en_;                                            // the next step's forcing, requested one step ahead
    sx_forcing_at(A, 0, kb, pn_, en_);
    int day_prev = day_index[0];
    for (int t = 0; t < A.nt; ++t) {
        const float prcp = pn_, pet = en_;
        const int day = day_index[t];                          // wave-uniform: scalar loads
        if (t + 1 < A.nt) sx_forcing_at(A, t + 1, kb, pn_, en_);
        if (day != day_prev) {                                 // a day is complete
            daily = daily + fminf(day_p, day_e);
            day_p = 0.f; day_e = 0.f; day_prev = day;
        }
        day_p = day_p + prcp;
        day_e = day_e + pet;
#pragma unroll
        for (int j = 0; j < SX_ICI_PER; ++j) {
            float ec;
            sx_interception_ieee(prcp, pet, cmax[j], h[j], ec);
            sum[j] = sum[j] + ec;
        }
    }
    daily = daily + fminf(day_p, day_e);

    // minloc: the first minimum, first within the thread's candidates, then over the rows in candidate order
    float best = 0.f; int besti = -1;
#pragma unroll
    for (int j = 0; j < SX_ICI_PER; ++j) {
        const float d = fabsf(sum[j] - daily);
        if (c0 + j < nc && (besti < 0 || d < best)) { best = d; besti = c0 + j; }
    }
    s_diff[threadIdx.y][threadIdx.x] = best;
    s_idx[threadIdx.y][threadIdx.x] = besti;
    __syncthreads();
    if (threadIdx.y == 0 && live) {
        for (int r = 1; r < (int)blockDim.y; ++r) {
            const float d = s_diff[r][threadIdx.x]; const int i = s_idx[r][threadIdx.x];
            if (i >= 0 && d < best) { best = d; besti = i; }
        }
        ci_out[k] = sx_ici_cmax(besti);
    }
}
