// sx_resident.h -- the catchment-resident forward kernel of smashx_uniform_costs (include/smashx_sbs.h): the small-S end of the
// ensemble path.  The candidates of a uniform calibration are a handful of runs on a small catchment (Cance: 383 cells x 1440 steps),
// where both the loop of forwards and the ensemble are launch latency on an empty card.  Here ONE workgroup holds the whole catchment
// of one sample, one thread per active cell, and ONE launch marches the whole period: reservoir levels and hlr never leave registers.
//
// Threads are ordered by level of the forest (the order / level tables of ens_tables) and time is skewed by level: at super-step u
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
// The arithmetic is that of the single run and of the ensemble, by construction: the vertical step IS sx_vertical_step<ST> /
// sx_vic_step, the routing statement is the one of sx_k_ens_route_fwd (sx_ensemble.h) with the upstream discharges summed in D8
// order, and the gauge series go to qg [g][t][SP] with the sample as column, where sx_k_ens_cost_gauge / sx_k_ens_cost_final fold them.
#pragma once

#include "sx_ensemble.h"

#define SX_RES_MAXCELLS 1024      // one cell per thread, one workgroup per sample

struct SxResTables {
    int nlevels;
    const int* cell;       // [n] plan cell of thread i (cells by level: ens_tables' order)
    const int* level;      // [n] its level
    const int* upline;     // [n][8] delay line of every upstream cell in D8 order: (first float << 5) | log2(slots); the first upn entries
    const int* upn;        // [n] by thread
    const int* ownline;    // [n] the thread's own line, same packing; -1: no downstream cell
    const int* gfirst;     // [n] first gauge on the thread's cell, -1: none
    const int* gnext;      // [ng] next gauge on the same cell, -1: none
};

// both values of step t of cell k, layout decided at run time: the values sx_forcing_at forms, read with per-lane addresses (the
// lanes of a wavefront are at different time steps here, so no row is wave-uniform).  Requesting step t + 1 before step t is
// computed was measured and dropped: no faster on Cance (2.0 us per super-step against 1.8), two more registers and 20 B of scratch per lane.
__device__ __forceinline__ void sx_res_forcing_at(const SxDeviceArrays& A, int t, int k, float& p, float& e) {
    const size_t npad = (size_t)A.npad;
    if (A.prcp16 == nullptr) { p = A.prcp[(size_t)t * npad + k]; e = A.pet[(size_t)t * npad + k]; return; }
    p = sx_prcp_decode(A, (unsigned)A.prcp16[(size_t)t * npad + k]);
    const int q = t + A.hour0;
    const float D = A.petd[(size_t)(q / 24) * npad + k];
    e = D < 0.f ? D : D * A.pet_ratio[q % 24];
}

extern __shared__ float sx_res_lines[];

// ST = 1..4: gr-a .. gr-d, 5: vic-a
template <int ST>
__global__ __launch_bounds__(SX_RES_MAXCELLS) void sx_k_res_fwd(SxDeviceArrays A, SxEnsArrays E, SxResTables R, int nt) {
    SX_LIBM_INIT();
    const int tid = threadIdx.x, s = blockIdx.x;
    const bool cell = tid < E.n;
    const int k = cell ? R.cell[tid] : 0;
    const int lev = cell ? R.level[tid] : 0;

    // per-thread parameters: the sample's value or the cell's base value (sx_ens_val with the roles of lane and cell swapped)
    SxCellParams P;
    SxVicParams V;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, cusl2_m4 = 0.f;      // gr: hi, hp, hft, hst; vic-a: husl1, husl2, hlsl
    if (ST == 5) {
        V.b = sx_ens_val(E, 0, k, s); V.cusl1 = sx_ens_val(E, 1, k, s); V.cusl2 = sx_ens_val(E, 2, k, s); V.clsl = sx_ens_val(E, 3, k, s);
        V.ks = sx_ens_val(E, 4, k, s); V.ds = sx_ens_val(E, 6, k, s); V.dsm = sx_ens_val(E, 7, k, s); V.ws = sx_ens_val(E, 8, k, s);
        sx_vic_derive(V);
        cusl2_m4 = sx_pow_m4(V.cusl2);
        h0 = sx_ens_val(E, SX_ENS_NP + 0, k, s); h1 = sx_ens_val(E, SX_ENS_NP + 1, k, s); h2 = sx_ens_val(E, SX_ENS_NP + 2, k, s);
    } else {
        P.ci = (ST == 2 || ST == 3) ? sx_ens_val(E, 0, k, s) : 1.f;
        P.cp = sx_ens_val(E, 1, k, s);
        P.cft = sx_ens_val(E, 2, k, s);
        P.cst = (ST == 3) ? sx_ens_val(E, 3, k, s) : 1.f;
        P.exc = (ST != 4) ? sx_ens_val(E, 4, k, s) : 0.f;
        sx_cell_params_init(P);
        P.cft_m4 = sx_pow_m4(P.cft);
        P.cst_m4 = (ST == 3) ? sx_pow_m4(P.cst) : 1.f;
        if (ST == 2 || ST == 3) h0 = sx_ens_val(E, SX_ENS_NP + 0, k, s);
        h1 = sx_ens_val(E, SX_ENS_NP + 1, k, s);
        h2 = sx_ens_val(E, SX_ENS_NP + 2, k, s);
        if (ST == 3) h3 = sx_ens_val(E, SX_ENS_NP + 3, k, s);
    }
    // routing invariants as sx_k_ens_route_fwd forms them; lr may be a sampled field, so rt_a is per thread
    const float lr = sx_ens_val(E, 5, k, s);
    const float a = sx_expf(-A.dt / (lr * 60.f));
    const int facc = A.flwacc[k];
    const float f = (float)(facc - 1);
    const float den = 0.001f * A.dx * A.dx * f;
    const bool hasup = facc > 1;
    const float dt = A.dt, dx = A.dx;
    const SxDiv dden = sx_mkdiv(den), ddt = sx_mkdiv(dt);
    float hlr = sx_ens_val(E, SX_ENS_NP + 4, k, s);

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
            sx_res_forcing_at(A, t, k, prcp, pet);
            if (ST == 5) qt = sx_vic_step(V, cusl2_m4, prcp, pet, h0, h1, h2);
            else {
                const bool still = SX_STILL && sx_wave_all(sx_is_still<(ST == 5 ? 1 : ST)>(prcp, pet, h0, h1));   // over the lanes in this branch
                qt = sx_vertical_step<(ST == 5 ? 1 : ST)>(P, prcp, pet, h0, h1, h2, h3, still);
            }
            // upstream discharges of step t in D8 order; "+ 0" for an absent upstream cell as in sx_k_ens_route_fwd
            const float v0 = nup > 0 ? sx_res_lines[(ul[0] >> 5) + (t & ((1 << (ul[0] & 31)) - 1))] : 0.f;
            const float v1 = nup > 1 ? sx_res_lines[(ul[1] >> 5) + (t & ((1 << (ul[1] & 31)) - 1))] : 0.f;
            float sum = v0 + v1;
#pragma unroll
            for (int c = 2; c < 8; ++c)
                if (c < nup) sum = sum + sx_res_lines[(ul[c] >> 5) + (t & ((1 << (ul[c] & 31)) - 1))];
            const float qup = hasup ? sx_div(sum * dt, dden) : 0.f;
            const float hr_imd = hlr + qup;
            const float hnew = hr_imd * a;
            const float qro = hr_imd - hnew;
            hlr = hnew;
            const float q = sx_div((qt + qro * f) * dx * dx * 0.001f, ddt);
            if (own >= 0) sx_res_lines[(own >> 5) + (t & ((1 << (own & 31)) - 1))] = q;
            for (int g = gfirst; g >= 0; g = R.gnext[g]) E.qg[((size_t)g * nt + t) * SP + s] = q;
        }
        __syncthreads();
    }
}
