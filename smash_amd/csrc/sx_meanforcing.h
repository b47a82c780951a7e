// sx_meanforcing.h -- mw_forcing_statistic::compute_mean_forcing (smash/solver/routine/mw_forcing_statistic.f90:18-75) on the forcing
// the plan holds in HBM: per gauge g and time step t, for prcp and pet independently,
//     mask = upstream(g) and value >= 0
//     mean = sum(value, mask) / real(count(mask))
// with the sum taken in fp32 over the cells in column-major order of the (nrow, ncol) grid, row index fastest, one addition after the
// other: the reference's result depends on that order, and set-up products are held to its bits.  count = 0 gives
// 0 / 0 = NaN, as there.  The division is the IEEE quotient in both builds.
//
// The sum over cells cannot be reassociated, so the parallelism is over (gauge, step) and nothing else: one LANE carries one
// (gauge, step) chain through the catchment's list of plan cells (sorted by column-major rank, built on the host: smashx.hip), a
// wavefront is 64 consecutive steps of one gauge.  The forcing rows are cell-fastest, so a lane's own values lie npad elements apart:
// read directly, every load would touch 64 lines for 64 values.  Hence the list goes in BLOCKS of 64 entries through LDS:
//   gather  row by row, lanes across the list entries: one load instruction fetches the 64 cells of the block at one step -- coalesced
//           wherever column-major neighbours are plan neighbours -- forms each value exactly as sx_forcing_at does (compact layout:
//           real(k) * prcp_c or the gap value; D < 0 ? D : D * ratio(hour), per cell, the ratio is NOT factored out of the sum) and
//           puts it into the tile at [step][entry].  An entry past the end of the list is stored as -1: the mask drops it.
//   walk    lane = step reads its own row of the tile in list order and adds: two independent chains per lane (prcp sum + count,
//           pet sum + count).
// A workgroup is SX_MF_WAVES wavefronts on ONE (gauge, 64 steps) chain: all of them gather (16 rows each), wavefront 0 also walks.  The
// tile is double-buffered: the loads of block b + 1 are issued, block b is walked while they are in flight, then they are stored and
// one barrier closes the block.  The tile is [64][64] with the column XOR-ed by the row (conflict-free both ways, no padding):
// 2 buffers x 2 fields x 16 KiB = 64 KiB of LDS per workgroup, two workgroups per compute unit.
// Daily PET of the compact layout changes every 24 steps: the 16 rows of a gathering wavefront lie in at most two days, so it loads two
// daily values per block instead of 16.
// The gather has NO branch between its loads (layout and wanted fields are template parameters, the day is a select): a wavefront's
// 16 - 32 loads of a block are all in flight at once.  With a wave-uniform branch per row (reload the daily PET when the day changes)
// the compiler waited for every load at the join and the rows went one memory latency after the other: twice the time.
// What was loaded is converted when it is stored into the tile, after the walk, so that nothing waits for it before.
//
// A launch covers list entries [j0, j0 + piece) of every gauge (SX_MF_PIECE, smashx.hip: bounded run time per launch); the running
// sums and counts travel between launches in a device buffer of their own, the launch that reaches the end of a gauge's list divides.
#pragma once

#include "sx_kernels.h"

#define SX_MF_WAVES 4                       // wavefronts per workgroup; 64 rows of a tile / SX_MF_WAVES rows per wavefront and block
#define SX_MF_ROWS (64 / SX_MF_WAVES)

struct SxMfState { float sum_p; int cnt_p; float sum_e; int cnt_e; };     // one (gauge, step) chain between two launches

// element [row][col] of a 64 x 64 tile
__device__ __forceinline__ int sx_mf_at(int row, int col) { return row * 64 + (col ^ row); }

// list[begin[g] .. begin[g + 1]): plan cells of gauge g's catchment in column-major order.  grid = (ceil(nt / 64), ng), block = 64 * SX_MF_WAVES.
// state[g * ntpad + t], ntpad = gridDim.x * 64; mean_p / mean_e (ng, nt) column-major; DO_P / DO_E false: that field is not read.
template <bool COMPACT, bool DO_P, bool DO_E>
__global__ __launch_bounds__(64 * SX_MF_WAVES, 2)      // two workgroups per compute unit, as the LDS allows
void sx_k_mean_forcing(SxDeviceArrays A, const int* __restrict__ list, const int* __restrict__ begin, int ng, int j0, int piece,
                       SxMfState* __restrict__ state, float* __restrict__ mean_p, float* __restrict__ mean_e) {
    static_assert(SX_MF_ROWS <= 24, "the rows of a gathering wavefront must lie in at most two days");
    __shared__ float s_tile[2][2][64 * 64];                    // [buffer][field][step][entry]
    const int g = blockIdx.y, t0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lb = begin[g], len = begin[g + 1] - lb;
    if (j0 >= len) return;                                     // this gauge was finished by an earlier launch (uniform over the workgroup; len >= 1)
    const int j1 = min(len, j0 + piece);
    const int nb = (j1 - j0 + 63) / 64;
    const size_t npad = (size_t)A.npad;
    const int r0 = wave * SX_MF_ROWS;                          // this wavefront gathers rows r0 .. r0 + SX_MF_ROWS - 1 of every tile
    // steps past the end repeat the last one and are not stored
    const int ta = min(t0 + r0, A.nt - 1), day_a = (ta + A.hour0) / 24, day_b = (min(t0 + r0 + SX_MF_ROWS - 1, A.nt - 1) + A.hour0) / 24;

    // block b of this launch as loaded: lane = list entry j0 + 64 b + lane, one row of the forcing per register (compact: the u16 count;
    // the daily PET of the first and of the last row's day)
    float vp[SX_MF_ROWS], ve[SX_MF_ROWS]; unsigned kp[SX_MF_ROWS]; float Da = 0.f, Db = 0.f; bool in = false;
    auto gather = [&](int b) {
        const int j = j0 + b * 64 + lane;
        in = j < j1;
        const size_t cell = (size_t)list[lb + (in ? j : j0)];
        if (COMPACT && DO_E) { Da = A.petd[(size_t)day_a * npad + cell]; Db = A.petd[(size_t)day_b * npad + cell]; }
#pragma unroll
        for (int r = 0; r < SX_MF_ROWS; ++r) {
            const int t = min(t0 + r0 + r, A.nt - 1);
            if (COMPACT) {
                if (DO_P) kp[r] = A.prcp16[(size_t)t * npad + cell];
            } else {
                if (DO_P) vp[r] = A.prcp[(size_t)t * npad + cell];
                if (DO_E) ve[r] = A.pet[(size_t)t * npad + cell];
            }
        }
    };
    // ... formed exactly as sx_forcing_at forms them and stored; an entry past the end of the list is -1
    auto put = [&](int buf) {
#pragma unroll
        for (int r = 0; r < SX_MF_ROWS; ++r) {
            float p = 0.f, e = 0.f;
            if (COMPACT) {
                if (DO_P) { const float v = (float)kp[r] * A.prcp_c; p = kp[r] == 65535u ? A.prcp_gap : v; }
                if (DO_E) {
                    const int q = min(t0 + r0 + r, A.nt - 1) + A.hour0;
                    const float D = q / 24 == day_a ? Da : Db;
                    e = D < 0.f ? D : D * ((sx_cfloat*)A.pet_ratio)[q % 24];
                }
            } else { if (DO_P) p = vp[r]; if (DO_E) e = ve[r]; }
            if (DO_P) s_tile[buf][0][sx_mf_at(r0 + r, lane)] = in ? p : -1.f;
            if (DO_E) s_tile[buf][1][sx_mf_at(r0 + r, lane)] = in ? e : -1.f;
        }
    };

    const int t = t0 + lane;                                   // wavefront 0: this lane's step
    const size_t si = (size_t)g * ((size_t)gridDim.x * 64) + (size_t)t;
    float sum_p = 0.f, sum_e = 0.f; int cnt_p = 0, cnt_e = 0;
    if (wave == 0 && j0 > 0) { const SxMfState s = state[si]; sum_p = s.sum_p; cnt_p = s.cnt_p; sum_e = s.sum_e; cnt_e = s.cnt_e; }

    gather(0); put(0);                                         // (nb >= 1: j0 < len)
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        const int buf = b & 1;
        if (b + 1 < nb) gather(b + 1);                         // in flight during the walk
        if (wave == 0) {
            if (DO_P) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const float v = s_tile[buf][0][sx_mf_at(lane, j)];
                    const bool m = v >= 0.f;
                    sum_p = m ? sum_p + v : sum_p;
                    cnt_p += m ? 1 : 0;
                }
            }
            if (DO_E) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const float v = s_tile[buf][1][sx_mf_at(lane, j)];
                    const bool m = v >= 0.f;
                    sum_e = m ? sum_e + v : sum_e;
                    cnt_e += m ? 1 : 0;
                }
            }
        }
        if (b + 1 < nb) put(buf ^ 1);
        __syncthreads();
    }
    if (wave != 0) return;
    if (j1 < len) {                                            // the list goes on in the next launch
        SxMfState s; s.sum_p = sum_p; s.cnt_p = cnt_p; s.sum_e = sum_e; s.cnt_e = cnt_e;
        state[si] = s;
        return;
    }
    if (t < A.nt) {
        const size_t o = (size_t)g + (size_t)t * ng;
        if (DO_P) mean_p[o] = sum_p / (float)cnt_p;            // the compiler's expansion of the IEEE division, as sx_interception_ieee
        if (DO_E) mean_e[o] = sum_e / (float)cnt_e;
    }
}
