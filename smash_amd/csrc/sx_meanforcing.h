// sx_meanforcing.h -- mw_forcing_statistic::compute_mean_forcing (smash/solver/routine/mw_forcing_statistic.f90:18-75) on the forcing
// the plan holds in HBM: per gauge g and time step t, for prcp and pet independently,
//     mask = upstream(g) and value >= 0
//     mean = sum(value, mask) / real(count(mask))
// with the sum taken in fp32 over the cells in column-major order of the (nrow, ncol) grid, row index fastest, one addition after the
// other: the reference's result depends on that order, and set-up products are held to its bits.  count = 0 gives
// 0 / 0 = NaN, as there.  The division is the IEEE quotient in both builds.
//
// The list (the catchment's plan cells sorted by column-major rank, built on the host: smashx.hip) goes through sx_listwalk.h; each
// value is formed per cell as sx_forcing_at forms it (the hourly ratio of the PET is NOT factored out of the sum), a padding entry is -1:
// the mask drops it.  The walk is two independent chains per lane (prcp sum + count, pet sum + count): 2 buffers x 2 fields x 16 KiB =
// 64 KiB of LDS per workgroup, two workgroups per compute unit.  Carried planes: sum_p, cnt_p, sum_e, cnt_e.
#pragma once

#include "sx_listwalk.h"

// one masked chain along this lane's row of a tile
__device__ __forceinline__ void sx_mf_chain(const float* tile, float& sum, int& cnt) {
    const int lane = threadIdx.x & 63;
#pragma unroll 16
    for (int j = 0; j < 64; ++j) {
        const float v = tile[sx_lw_at(lane, j)];
        const bool m = v >= 0.f;
        sum = m ? sum + v : sum;
        cnt += m ? 1 : 0;
    }
}

template <bool DO_P, bool DO_E>
struct SxMfWalk {
    float *state, *mean_p, *mean_e; int ng, nt;
    float sum_p = 0.f, sum_e = 0.f; int cnt_p = 0, cnt_e = 0;
    __device__ __forceinline__ float& field(int f) { return sx_lw_field(state, f, ng); }
    __device__ __forceinline__ void resume() {
        if (DO_P) { sum_p = field(0); cnt_p = __float_as_int(field(1)); }
        if (DO_E) { sum_e = field(2); cnt_e = __float_as_int(field(3)); }
    }
    __device__ __forceinline__ float gather(int) { return -1.f; }
    __device__ __forceinline__ void stored() {}
    __device__ __forceinline__ void walk(int, const float* rain, const float* pet) {
        if (DO_P) sx_mf_chain(rain, sum_p, cnt_p);
        if (DO_E) sx_mf_chain(pet, sum_e, cnt_e);
    }
    __device__ __forceinline__ void put_away() {
        if (DO_P) { field(0) = sum_p; field(1) = __int_as_float(cnt_p); }
        if (DO_E) { field(2) = sum_e; field(3) = __int_as_float(cnt_e); }
    }
    __device__ __forceinline__ void close() {
        const int t = blockIdx.x * 64 + (threadIdx.x & 63);
        if (t >= nt) return;
        const size_t o = (size_t)blockIdx.y + (size_t)t * ng;
        if (DO_P) mean_p[o] = sum_p / (float)cnt_p;            // the compiler's expansion of the IEEE division, as sx_interception_ieee
        if (DO_E) mean_e[o] = sum_e / (float)cnt_e;
    }
};

// list[begin[g] .. begin[g + 1]): gauge g's list in whole blocks.  grid = (ceil(nt / 64), ng), block = 64 * SX_LW_WAVES.
// state (4, ng, ntpad), ntpad = gridDim.x * 64; mean_p / mean_e (ng, nt) column-major; DO_P / DO_E false: that field is not read.
template <bool COMPACT, bool DO_P, bool DO_E>
__global__ __launch_bounds__(64 * SX_LW_WAVES, 2)      // two workgroups per compute unit, as the LDS allows
void sx_k_mean_forcing(SxDeviceArrays A, const int* __restrict__ list, const int* __restrict__ begin, int ng, int b0, int nbp,
                       float* __restrict__ state, float* __restrict__ mean_p, float* __restrict__ mean_e) {
    const int lb = begin[blockIdx.y];
    SxMfWalk<DO_P, DO_E> w{state, mean_p, mean_e, ng, A.nt};
    sx_listwalk<COMPACT, DO_P, DO_E, 2>(A, list + lb, (begin[blockIdx.y + 1] - lb) / 64, b0, nbp, w);
}
