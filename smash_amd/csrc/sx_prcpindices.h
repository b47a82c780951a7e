// sx_prcpindices.h -- mw_forcing_statistic::compute_prcp_indices (smash/solver/routine/mw_forcing_statistic.f90:77-220) on the rain the
// plan holds in HBM: per gauge g and time step t, with d = flwdst - flwdst(gauge) (host side, with its quantiles flwdst_qtl and the
// cumulated bin counts wf: sx_tablehost.h),
//     mask   = upstream(g) and rain >= 0;  n = count(mask);  minv_n = 1 / real(n)
//     sum_p, sum_p2, sum_d, sum_d2, sum_pd, sum_pd2 = sums over mask of m, m*m, d, d*d, m*d, (m*d)*d
//     sum_b(k) = sum of the rain over { flwdst_qtl(k-1) < d <= flwdst_qtl(k) } of the WHOLE grid, gap values as they are, k = 2 .. 11
// every sum sequential in fp32 over the cells in column-major order, one addition after the other, no product contracted into an
// addition: the reference's result depends on that order, and set-up products are held to its bits.  Then, on the steps
// with sum_p > 0 only, the closing arithmetic (sx_pi_close below) with IEEE divisions and square root in both builds.
//
// A gauge's work is ONE list through sx_listwalk.h: section 0 is the catchment, sections 1 .. 10 the ten distance bins, every section
// padded to whole blocks, so that a block belongs to one section.  A padding entry becomes -1 in the catchment (the mask drops it) and
// +0 in a bin (x + 0 = x for every x a sum that starts at +0 can hold).  The walk:
//   catchment  the count and six sums, six independent dependency chains; d and d*d of the entry are wave-uniform: the walking lanes
//              hold the block's 64 distances one per lane (loaded with the block's gather) and read entry j's with v_readlane
//   bin        one plain sum; at the last block of a bin it is put away in the state buffer
// Carried planes: count, six sums, the open bin sum, ten finished bin sums.  The lane that walks a gauge's last block closes: it reads
// its ten bin sums back, the rain of the cell (gauge_row, gauge_row) at its step -- the reference indexes the column with the gauge's
// ROW (mw_forcing_statistic.f90:181) --, and writes (std, d1, d2, vg) and a flag; the host copies the flagged pairs only, the others
// stay as the caller passed them.
#pragma once

#include "sx_listwalk.h"
#include "sx_tables.h"                      // SX_PI_NQ, SxPiGauge

#define SX_PI_NF 18                         // state fields: count, six sums, the open bin sum, ten finished bin sums

__device__ __forceinline__ float sx_pi_uniform(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

// the closing arithmetic of one (gauge, step) with sum_p > 0, every operation rounded on its own
__device__ __forceinline__ void sx_pi_close(const SxPiGauge& G, int n, float sum_p, float sum_p2, float sum_d, float sum_d2, float sum_pd, float sum_pd2,
                                            float pcell, const float* bsum, float* res) {
    const float minv_n = 1.f / (float)n;
    const float mean_p = __fmul_rn(minv_n, sum_p), p0 = mean_p;
    const float p1 = __fmul_rn(minv_n, sum_pd), p2 = __fmul_rn(minv_n, sum_pd2), g1 = __fmul_rn(minv_n, sum_d), g2 = __fmul_rn(minv_n, sum_d2);
    float pwf[SX_PI_NQ];
    { const float q = pcell / sum_p; pwf[0] = q > 0.f ? q : 0.f; }
#pragma unroll
    for (int k = 1; k < SX_PI_NQ; ++k) {
        const float mean_subp = G.cnt[k] == 0.f ? 0.f : bsum[k] / G.cnt[k];
        pwf[k] = __fadd_rn(pwf[k - 1], __fmul_rn(mean_subp / mean_p, G.wf[k]));
    }
    const float d1 = p1 / __fmul_rn(p0, g1);
    const float a = p1 / p0;
    const float d2 = __fmul_rn(1.f / __fsub_rn(g2, __fmul_rn(g1, g1)), __fsub_rn(p2 / p0, __fmul_rn(a, a)));
    const float sd = sqrtf(__fsub_rn(__fmul_rn(minv_n, sum_p2), __fmul_rn(mean_p, mean_p)));
    // maxval as the compiled reference forms it: the first element, replaced where the next one compares greater
    float vg = 0.f;
#pragma unroll
    for (int k = 0; k < SX_PI_NQ; ++k) {
        const float x = fabsf(__fsub_rn(pwf[k] / pwf[SX_PI_NQ - 1], G.wf[k] / G.wf[SX_PI_NQ - 1]));
        vg = (k == 0 || x > vg) ? x : vg;
    }
    res[0] = sd; res[1] = d1; res[2] = d2; res[3] = vg;
}

template <bool COMPACT>
struct SxPiWalk {
    const SxDeviceArrays& A; const SxPiGauge& G; const float *dl, *d2l; float *state, *out; int* flag; int ng;
    const int sec1 = G.sec[1];                                 // blocks of the catchment
    int n = 0; float sum_p = 0.f, sum_p2 = 0.f, sum_d = 0.f, sum_d2 = 0.f, sum_pd = 0.f, sum_pd2 = 0.f, bs = 0.f;
    int s = 0;                                                 // the section of the block being walked
    float dn = 0.f, d2n = 0.f, dc = 0.f, d2c = 0.f;            // wavefront 0: the distances of the block loaded last and of the one in the tile, lane = entry
    __device__ __forceinline__ float& field(int f) { return sx_lw_field(state, f, ng); }
    __device__ __forceinline__ void resume() {
        n = __float_as_int(field(0));
        sum_p = field(1); sum_p2 = field(2); sum_d = field(3); sum_d2 = field(4); sum_pd = field(5); sum_pd2 = field(6); bs = field(7);
    }
    __device__ __forceinline__ float gather(int b) {
        if (threadIdx.x < 64 && b < sec1) { const size_t i = (size_t)G.db + (size_t)b * 64 + threadIdx.x; dn = dl[i]; d2n = d2l[i]; }
        return b < sec1 ? -1.f : 0.f;
    }
    __device__ __forceinline__ void stored() { dc = dn; d2c = d2n; }
    __device__ __forceinline__ void walk(int b, const float* rain, const float*) {
        const int lane = threadIdx.x & 63;
        if (b < sec1) {
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const float v = rain[sx_lw_at(lane, j)];
                const float d = sx_pi_uniform(dc, j), d2 = sx_pi_uniform(d2c, j);
                const bool m = v >= 0.f;
                const float vd = __fmul_rn(v, d);
                n += m ? 1 : 0;
                sum_p = m ? __fadd_rn(sum_p, v) : sum_p;
                sum_p2 = m ? __fadd_rn(sum_p2, __fmul_rn(v, v)) : sum_p2;
                sum_d = m ? __fadd_rn(sum_d, d) : sum_d;
                sum_d2 = m ? __fadd_rn(sum_d2, d2) : sum_d2;
                sum_pd = m ? __fadd_rn(sum_pd, vd) : sum_pd;
                sum_pd2 = m ? __fadd_rn(sum_pd2, __fmul_rn(vd, d)) : sum_pd2;
            }
        } else {
            while (b >= G.sec[s + 1]) ++s;                     // wave-uniform; empty bins are passed over
#pragma unroll 16
            for (int j = 0; j < 64; ++j) bs = __fadd_rn(bs, rain[sx_lw_at(lane, j)]);
            if (b + 1 == G.sec[s + 1]) { field(7 + s) = bs; bs = 0.f; }      // the bin is complete
        }
    }
    __device__ __forceinline__ void put_away() {
        field(0) = __int_as_float(n);
        field(1) = sum_p; field(2) = sum_p2; field(3) = sum_d; field(4) = sum_d2; field(5) = sum_pd; field(6) = sum_pd2; field(7) = bs;
    }
    __device__ __forceinline__ void close() {
        const int t = blockIdx.x * 64 + (threadIdx.x & 63);
        if (t >= A.nt) return;
        const size_t o = (size_t)blockIdx.y + (size_t)t * ng;
        if (!(sum_p > 0.f)) { flag[o] = 0; return; }           // no rain: the caller's entries stay
        float bsum[SX_PI_NQ];
        bsum[0] = 0.f;
#pragma unroll
        for (int k = 1; k < SX_PI_NQ; ++k) bsum[k] = G.cnt[k] == 0.f ? 0.f : field(7 + k);
        const size_t i = (size_t)t * (size_t)A.npad + (size_t)G.krr;
        const float pcell = COMPACT ? sx_prcp_decode(A, A.prcp16[i]) : A.prcp[i];
        float res[4];
        sx_pi_close(G, n, sum_p, sum_p2, sum_d, sum_d2, sum_pd, sum_pd2, pcell, bsum, res);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[o * 4 + k] = res[k];
        flag[o] = 1;
    }
};

// grid = (ceil(nt / 64), ng), block = 64 * SX_LW_WAVES.  list: plan cells or -1; dl / d2l: d and d*d of the catchment entries;
// state (SX_PI_NF, ng, ntpad), ntpad = gridDim.x * 64; out (4, ng, nt) column-major; flag (ng, nt): 1 where out was written.
template <bool COMPACT>
__global__ __launch_bounds__(64 * SX_LW_WAVES, 2)
void sx_k_prcp_indices(SxDeviceArrays A, const int* __restrict__ list, const float* __restrict__ dl, const float* __restrict__ d2l,
                       const SxPiGauge* __restrict__ gauges, int ng, int b0, int nbp, float* __restrict__ state, float* __restrict__ out,
                       int* __restrict__ flag) {
    const SxPiGauge& G = gauges[blockIdx.y];
    SxPiWalk<COMPACT> w{A, G, dl, d2l, state, out, flag, ng};
    sx_listwalk<COMPACT, true, false, 1>(A, list + G.lb, G.sec[SX_PI_NQ], b0, nbp, w);
}
