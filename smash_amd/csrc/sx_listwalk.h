// sx_listwalk.h -- the machine under the catchment statistics of the resident forcing (sx_meanforcing.h, sx_prcpindices.h).
// Their sums are sequential in fp32 over a list of cells, so the parallelism is over (gauge, step) and nothing else: one LANE carries
// one (gauge, step) chain through the gauge's list of plan cells, a wavefront is 64 consecutive steps of one gauge, a workgroup is
// SX_LW_WAVES wavefronts on ONE such chain.  The forcing rows are cell-fastest, so a lane's own values lie npad elements apart; hence the
// list goes in BLOCKS of 64 entries (the host pads it to whole blocks with the entry -1) through a 64 x 64 LDS tile [step][entry]:
//   gather  all wavefronts, SX_LW_ROWS rows each, lanes across the entries: one load instruction fetches the 64 cells of the block at
//           one step.  NO branch between the loads (layout and fields are template parameters, the day of the daily PET is a select
//           between the days of the wavefront's first and last row): a wavefront's 16 - 32 loads of a block are all in flight at once;
//           with a wave-uniform branch per row the compiler waits for every load at the join: twice the time.
//   walk    wavefront 0, lane = step, along its row in list order: the kernel's own code.
// The tile is double-buffered: the loads of block b + 1 are issued, block b is walked while they are in flight, then they are formed
// exactly as sx_forcing_at forms them and stored (after the walk, so that nothing waits for them before), one barrier closes the block.
// The column is XOR-ed with the row: conflict-free both ways, no padding.  A padding entry is stored as the value the kernel names for
// its block.  A launch covers blocks [b0, b0 + nbp) of every gauge (bounded run time per launch); what the chains hold travels between
// launches in planes [field][gauge][step] of a plan buffer, the launch that reaches the end of a gauge's list closes.
#pragma once

#include "sx_kernels.h"

#define SX_LW_WAVES 4                       // wavefronts per workgroup; 64 rows of a tile / SX_LW_WAVES rows per wavefront and block
#define SX_LW_ROWS (64 / SX_LW_WAVES)

// element [row][col ^ row] of a 64 x 64 tile, row and col in 0 .. 63: row * 64 + (col ^ row), written as one XOR on a value per row
__device__ __forceinline__ int sx_lw_at(int row, int col) { return (row * 65) ^ col; }

// plane f of the carried state at this lane's (gauge, step); grid = (ceil(nt / 64), ng)
__device__ __forceinline__ float& sx_lw_field(float* state, int f, int ng) {
    return state[((size_t)f * ng + blockIdx.y) * ((size_t)gridDim.x * 64) + (size_t)(blockIdx.x * 64 + (threadIdx.x & 63))];
}

// Blocks [b0, b0 + nbp) of the list (nblk blocks, plan cells or -1) through the tile; block = 64 * SX_LW_WAVES, NFLD tiles per buffer
// (rain in the first, PET in the second).  W, used by wavefront 0 except for gather():
//   resume()               b0 > 0: take the chains up where the previous launch put them away
//   gather(b) -> float     every wavefront, among the loads of block b: loads of W's own; returns what a padding entry is stored as
//   stored()               block b's loads are in the tile, the next gather() may overwrite what the last one loaded
//   walk(b, rain, pet)     this lane's row of block b: tile[sx_lw_at(lane, j)], j = 0 .. 63
//   put_away() / close()   the list goes on in the next launch / is done
template <bool COMPACT, bool DO_P, bool DO_E, int NFLD, class W>
__device__ __forceinline__ void sx_listwalk(const SxDeviceArrays& A, const int* __restrict__ list, int nblk, int b0, int nbp, W& w) {
    static_assert(SX_LW_ROWS <= 24, "the rows of a gathering wavefront must lie in at most two days");
    __shared__ float s_tile[2][NFLD][64 * 64];                 // [buffer][field][step][entry]
    if (b0 >= nblk) return;                                    // this gauge was finished by an earlier launch (uniform over the workgroup)
    const int b1 = min(nblk, b0 + nbp);
    const int t0 = blockIdx.x * 64, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t npad = (size_t)A.npad;
    const int r0 = wave * SX_LW_ROWS;                          // this wavefront gathers rows r0 .. r0 + SX_LW_ROWS - 1 of every tile
    // steps past the end repeat the last one and are not stored
    const int day_a = (min(t0 + r0, A.nt - 1) + A.hour0) / 24, day_b = (min(t0 + r0 + SX_LW_ROWS - 1, A.nt - 1) + A.hour0) / 24;

    // a block as loaded: lane = entry, one row of the forcing per register (compact: the u16 count; the daily PET of the two days)
    float vp[SX_LW_ROWS], ve[SX_LW_ROWS]; unsigned kp[SX_LW_ROWS]; float Da = 0.f, Db = 0.f, padv = 0.f; bool in = false;
    auto gather = [&](int b) {
        const int c = list[(size_t)b * 64 + lane];
        in = c >= 0;
        padv = w.gather(b);
        const size_t cell = (size_t)(in ? c : 0);
        if (COMPACT && DO_E) { Da = A.petd[(size_t)day_a * npad + cell]; Db = A.petd[(size_t)day_b * npad + cell]; }
#pragma unroll
        for (int r = 0; r < SX_LW_ROWS; ++r) {
            const int t = min(t0 + r0 + r, A.nt - 1);
            if (COMPACT) {
                if (DO_P) kp[r] = A.prcp16[(size_t)t * npad + cell];
            } else {
                if (DO_P) vp[r] = A.prcp[(size_t)t * npad + cell];
                if (DO_E) ve[r] = A.pet[(size_t)t * npad + cell];
            }
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int r = 0; r < SX_LW_ROWS; ++r) {
            float p = 0.f, e = 0.f;
            if (COMPACT) {
                if (DO_P) p = sx_prcp_decode(A, kp[r]);
                if (DO_E) {
                    const int q = min(t0 + r0 + r, A.nt - 1) + A.hour0;
                    const float D = q / 24 == day_a ? Da : Db;
                    e = D < 0.f ? D : D * ((sx_cfloat*)A.pet_ratio)[q % 24];
                }
            } else { if (DO_P) p = vp[r]; if (DO_E) e = ve[r]; }
            if (DO_P) s_tile[buf][0][sx_lw_at(r0 + r, lane)] = in ? p : padv;
            if (DO_E) s_tile[buf][NFLD - 1][sx_lw_at(r0 + r, lane)] = in ? e : padv;
        }
    };

    if (wave == 0 && b0 > 0) w.resume();
    gather(b0); put(0);
    w.stored();
    __syncthreads();
    for (int b = b0; b < b1; ++b) {
        const int buf = (b - b0) & 1;
        if (b + 1 < b1) gather(b + 1);                         // in flight during the walk
        if (wave == 0) w.walk(b, s_tile[buf][0], s_tile[buf][NFLD - 1]);
        if (b + 1 < b1) put(buf ^ 1);
        w.stored();
        __syncthreads();
    }
    if (wave != 0) return;
    if (b1 < nblk) w.put_away();
    else w.close();
}
