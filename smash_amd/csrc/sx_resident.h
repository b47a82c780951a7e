// sx_resident.h -- the catchment-resident forward kernel of smashx_uniform_costs (include/smashx_sbs.h): the small-S end of the
// ensemble path.  The candidates of a uniform calibration are a handful of runs on a small catchment (Cance: 383 cells x 1440 steps),
// where both the loop of forwards and the ensemble are launch latency on an empty card.  Here ONE workgroup holds the whole catchment
// of one sample, one thread per active cell, and ONE launch marches the whole period: reservoir levels and hlr never leave registers.
//
// Threads are ordered by level of the forest (the order / level tables of sx_forest, sx_tablehost.h) and time is skewed by level: at super-step u
// the cell of level l does its step t = u - l, if 0 <= t < nt.  Every upstream cell of a cell lies in a lower level, so its discharge
// of step t was written at an earlier super-step (t + l_up < t + l_down): one __syncthreads() per super-step is the dependency,
// nt + nlevels - 1 super-steps in all.  No flags, no spinning, no atomics; every thread of the block reaches every barrier, idle
// ones included, and the trip count is uniform.
//
// The hand-off lives in LDS: the discharge a cell hands down is written at super-step t + l_up and read at t + l_down, D = l_down -
// l_up super-steps later, so every cell with a downstream cell owns a delay line, a ring indexed by t.  With one barrier per
// super-step a ring of D slots is one too short: the read of step t and the write of step t + D fall into the SAME super-step on
// different threads, with no barrier between them.  D + 1 slots separate them by a barrier, and the ring is rounded up to a power
// of two so that the slot is t & mask (D = 1, by far the most frequent, costs 2 floats; the host refuses what does not fit).
//
// The arithmetic is that of the single run and of the ensemble, by construction: the cell set-up, the vertical step, the forcing
// decode (sx_forcing_at, here with per-lane addresses) and the routing step (sx_route_cell / sx_route_step, the upstream discharges
// summed in D8 order) are the functions sx_k_ens_vert_fwd / sx_k_ens_route_fwd call (sx_ensemble.h), and the gauge series go to qg
// [g][t][SP] with the sample as column, where sx_k_ens_cost_gauge / sx_k_ens_cost_final fold them.
// Requesting the forcing of step t + 1 before step t is computed was measured and dropped: no faster on Cance (2.0 us per super-step
// against 1.8), two more registers and 20 B of scratch per lane.
#pragma once

#include "sx_ensemble.h"
#include "sx_tables.h"            // SX_RES_MAXCELLS

struct SxResTables {
    int nlevels;
    const int* cell;       // [n] plan cell of thread i (cells by level: sx_forest's order)
    const int* level;      // [n] its level
    const int* upline;     // [n][8] delay line of every upstream cell in D8 order: (first float << 5) | log2(slots); the first upn entries
    const int* upn;        // [n] by thread
    const int* ownline;    // [n] the thread's own line, same packing; -1: no downstream cell
    const int* gfirst;     // [n] first gauge on the thread's cell, -1: none
    const int* gnext;      // [ng] next gauge on the same cell, -1: none
};

extern __shared__ float sx_res_lines[];

// ST = 1..4: gr-a .. gr-d, 5: vic-a
template <int ST>
__global__ __launch_bounds__(SX_RES_MAXCELLS) void sx_k_res_fwd(SxDeviceArrays A, SxEnsArrays E, SxResTables R, int nt) {
    SX_LIBM_INIT();
    const int tid = threadIdx.x, s = blockIdx.x;
    const bool cell = tid < E.n;
    const int k = cell ? R.cell[tid] : 0;
    const int lev = cell ? R.level[tid] : 0;

    // per-thread parameters: the sample's value or the cell's base value (sx_k_ens_vert_fwd's source, captured by value like there,
    // with the roles of lane and cell swapped); the initial levels come from the same source
    const auto val = [=](int slot) { return sx_ens_val(E, slot, k, s); };
    SxCellParams P;
    SxVicParams V;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, cusl2_m4 = 0.f;      // gr: hi, hp, hft, hst; vic-a: husl1, husl2, hlsl
    if constexpr (ST == 5) {
        V = sx_vic_params(val);
        cusl2_m4 = sx_pow_m4(V.cusl2);
        sx_vic_levels_in(val, h0, h1, h2);
    } else {
        sx_cell_params<ST>(val, P);
        sx_fwd_powers<ST>(P);
        sx_levels_in<ST>(val, h0, h1, h2, h3);
    }
    const SxRouteCell C = sx_route_cell(A, val(SX_SLOT_LR), k);      // lr may be a sampled field, so rt_a is per thread
    float hlr = val(SX_SLOT_HLR);

    const int nup = cell ? R.upn[tid] : 0;
    int ul[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) ul[c] = (cell && c < nup) ? R.upline[(size_t)tid * 8 + c] : 0;
    const int own = cell ? R.ownline[tid] : -1;
    const int gfirst = cell ? R.gfirst[tid] : -1;
    const size_t SP = (size_t)E.SP;

    const int nsuper = nt + R.nlevels - 1;
    for (int u = 0; u < nsuper; ++u) {
        const int t = u - lev;
        if (cell && t >= 0 && t < nt) {
            float prcp, pet, qt;
            sx_forcing_at<false>(A, t, k, prcp, pet);      // the lanes of a wavefront are at different steps: no row is wave-uniform
            if constexpr (ST == 5) qt = sx_vic_step(V, cusl2_m4, prcp, pet, h0, h1, h2);
            else {
                const bool still = SX_STILL && sx_wave_all(sx_is_still<ST>(prcp, pet, h0, h1));   // over the lanes in this branch
                qt = sx_vertical_step<ST>(P, prcp, pet, h0, h1, h2, h3, still);
            }
            // upstream discharges of step t in D8 order; "+ 0" for an absent upstream cell as in sx_k_ens_route_fwd
            const float v0 = nup > 0 ? sx_res_lines[(ul[0] >> 5) + (t & ((1 << (ul[0] & 31)) - 1))] : 0.f;
            const float v1 = nup > 1 ? sx_res_lines[(ul[1] >> 5) + (t & ((1 << (ul[1] & 31)) - 1))] : 0.f;
            float sum = v0 + v1;
#pragma unroll
            for (int c = 2; c < 8; ++c)
                if (c < nup) sum = sum + sx_res_lines[(ul[c] >> 5) + (t & ((1 << (ul[c] & 31)) - 1))];
            const float q = sx_route_step(C, sum, qt, hlr);
            if (own >= 0) sx_res_lines[(own >> 5) + (t & ((1 << (own & 31)) - 1))] = q;
            for (int g = gfirst; g >= 0; g = R.gnext[g]) E.qg[((size_t)g * nt + t) * SP + s] = q;
        }
        __syncthreads();
    }
}
