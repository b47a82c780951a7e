// sx_ensemble.h -- kernels of the ensemble path: S forward runs that differ only in a handful of spatially uniform parameter /
// initial-state values (compute_multiple_run, smash/solver/routine/mw_multiple_run.f90:40-119), computed at once.
//
// Layout rule: the SAMPLE index is fastest everywhere, padded to 64, so a wavefront is 64 samples of ONE cell and every load / store
// of per-sample data is one contiguous 256-B row:
//   sample       [nfields][SP]           the sampled values of the batch (columns past the last sample repeat it)
//   base         [14][npad]              the caller's fields in cell order: parameter slots 0..8, state slots 9..13 (smashx.hip)
//   state        [5][n][SP]              running reservoir levels, so that the next time chunk resumes
//   qt           [n][Tc][SP]             lateral inflow of a time chunk; the routing kernel writes the discharge q over it in place
//   qg           [ng][nt][SP]            discharge at the gauges over the whole period (cost, res_qsim)
// The forcing of a cell-step is ONE value per wavefront (a broadcast load from the plan's resident rows, whatever their layout), and
// the wave-uniform still-step shortcut of sx_ops.h fires on the forcing alone.
//
// The arithmetic is that of the single run, by construction: the cell is set up by the functions the single run's kernels call
// (sx_cell_params, sx_fwd_powers, sx_levels_in / _out, sx_vic_params: sx_ops.h, sx_vic.h) from another field source, the vertical
// step IS sx_vertical_step<ST> / sx_vic_step, the routing is sx_route_cell / sx_route_step (sx_ops.h), whose invariants
// sx_k_prep_routing stores for the group kernels, and the cost folds the gauge series through sx_sums_add / sx_gauge_jobs of
// sx_cost.h, the functions sx_k_cost_sums / sx_k_cost_final call.  One statement is still restated: sx_route_step says in scalars
// what sx_route_fwd_group (sx_kernels.h, TMODE 0) says on float4 time blocks behind its LDS exchange, because a function carved
// out of the group kernel's body would change its schedule.
#pragma once

#include "sx_cost.h"
#include "sx_kernels.h"

#define SX_ENS_CELLS 4       // cells (= wavefronts) per vertical workgroup

struct SxEnsArrays {
    int n, npad, SP, Tc;
    const float* base;
    const float* sample;
    int smap[SX_NSLOTS];         // row of `sample` that replaces the slot, -1: the base field
    float* state;
    float* qt;
    const int* up;               // [n][8] upstream cells in D8 order 1..8 (md_routing_operator.f90:37-53), the first upn[k] entries
    const int* upn;              // [n]
    const int* order;            // [n] cells by level of the forest: every upstream cell of a level's cells lies in an earlier level
    float* qg;
    const int* gauge_k;          // [ng] cell of every gauge
    float* gj;                   // [ng][SP] gauge_jobs
    float* med;                  // [ng][SP] scratch of the median over the negative-weight gauges
    float* cost;                 // [SP]
    float* qout;                 // [SP][nt][ng]: res_qsim of the batch, gauge fastest
};

// the value of field slot `slot` for (cell k, sample column s): the lane's sample or the cell's base value
__device__ __forceinline__ float sx_ens_val(const SxEnsArrays& E, int slot, int k, int s) {
    const int r = E.smap[slot];
    return r >= 0 ? E.sample[(size_t)r * E.SP + s] : E.base[(size_t)slot * E.npad + k];
}

// initial states of a batch: [slot][cell][sample]
__global__ __launch_bounds__(64) void sx_k_ens_init_states(SxEnsArrays E, int used_mask) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    for (int k = blockIdx.y; k < E.n; k += gridDim.y) {
#pragma unroll
        for (int i = 0; i < SX_NSSLOTS; ++i)
            if (used_mask >> i & 1) E.state[((size_t)i * E.n + k) * E.SP + s] = sx_ens_val(E, SX_SLOT_HI + i, k, s);
    }
}

// ------------------------------------------------------------------------------------------------
// vertical forward: one thread per (cell, sample) marches the time chunk [t0, t0 + T).  ST = 1..4: gr-a .. gr-d, 5: vic-a
// ------------------------------------------------------------------------------------------------
template <int ST>
__global__ __launch_bounds__(64 * SX_ENS_CELLS) void sx_k_ens_vert_fwd(SxDeviceArrays A, SxEnsArrays E, int t0, int T) {
    SX_LIBM_INIT();      // exact-libm build: the tables of expf / logf / powf into LDS (sx_libm.h); nothing otherwise
    const int s = blockIdx.x * 64 + threadIdx.x;
    const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * SX_ENS_CELLS + threadIdx.y));     // one cell per wavefront
    if (k >= E.n) return;
    const size_t SP = (size_t)E.SP, nS = (size_t)E.n * SP;
    // the ensemble's field source (sx_ops.h).  Captured by value: behind a captured reference to E the select of sx_ens_val stays a
    // branch per field (40 to 70 instructions more per kernel, two registers more in sx_k_res_fwd)
    const auto val = [=](int slot) { return sx_ens_val(E, slot, k, s); };
    float* sv = E.state + (size_t)k * SP + s;                // the running levels are a source and a sink of their own
    const auto lev = [=](int slot) { return sv[(size_t)(slot - SX_SLOT_HI) * nS]; };
    const auto lev_out = [=](int slot, float h) { sv[(size_t)(slot - SX_SLOT_HI) * nS] = h; };

    SxCellParams P;
    SxVicParams V;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, cusl2_m4 = 0.f;      // gr: hi, hp, hft, hst; vic-a: husl1, husl2, hlsl
    if constexpr (ST == 5) {
        V = sx_vic_params(val);
        cusl2_m4 = sx_pow_m4(V.cusl2);
        sx_vic_levels_in(lev, h0, h1, h2);
    } else {
        sx_cell_params<ST>(val, P);
        sx_fwd_powers<ST>(P);
        sx_levels_in<ST>(lev, h0, h1, h2, h3);
    }
    const unsigned kb = (unsigned)k * 4u;
    float* q = E.qt + (size_t)k * E.Tc * SP + s;
    for (int tt = 0; tt < T; ++tt) {
        float prcp, pet;
        sx_forcing_at(A, t0 + tt, kb, prcp, pet);            // wave-uniform address: one value per wavefront
        if constexpr (ST == 5) q[(size_t)tt * SP] = sx_vic_step(V, cusl2_m4, prcp, pet, h0, h1, h2);
        else {
            const bool still = SX_STILL && sx_wave_all(sx_is_still<ST>(prcp, pet, h0, h1));
            q[(size_t)tt * SP] = sx_vertical_step<ST>(P, prcp, pet, h0, h1, h2, h3, still);
        }
    }
    if constexpr (ST == 5) sx_vic_levels_out(lev_out, h0, h1, h2);
    else sx_levels_out<ST>(lev_out, h0, h1, h2, h3);
}

// ------------------------------------------------------------------------------------------------
// routing forward, TIME INNERMOST: one thread per (cell of one level of the forest, sample) routes the whole chunk.  Legal because
// a cell only reads the current-step discharge of its upstream cells (md_routing_operator.f90:35-56) and those lie in earlier
// levels, i.e. in launches that have completed: q[up][t] is final for every t of the chunk.  None of the loads depends on a value
// computed in the loop (only hlr is carried), so a block of SX_ENS_RB steps is requested at once; no LDS, no barrier.
// upstream_discharge + linear_routing + the q update of md_forward_structure.f90:150-156 in the reference's operation order.
// ------------------------------------------------------------------------------------------------
#define SX_ENS_RB 4
__global__ __launch_bounds__(64) void sx_k_ens_route_fwd(SxDeviceArrays A, SxEnsArrays E, int i0, int T) {
    SX_LIBM_INIT();
    const int s = blockIdx.x * 64 + threadIdx.x;
    const int k = __builtin_amdgcn_readfirstlane(E.order[i0 + (int)blockIdx.y]);
    const size_t SP = (size_t)E.SP, row = (size_t)E.Tc * SP;
    const SxRouteCell R = sx_route_cell(A, sx_ens_val(E, SX_SLOT_LR, k, s), k);      // lr may be a sampled field, so rt_a is per lane
    float* hl = E.state + ((size_t)(SX_SLOT_HLR - SX_SLOT_HI) * E.n + k) * SP + s;
    float hlr = *hl;
    const int nup = __builtin_amdgcn_readfirstlane(E.upn[k]);
    const int* upk = E.up + (size_t)k * 8;
    float* q = E.qt + (size_t)k * row + s;
    const float* u0 = E.qt + (size_t)(nup > 0 ? upk[0] : k) * row + s;
    const float* u1 = E.qt + (size_t)(nup > 1 ? upk[1] : k) * row + s;
    for (int tb = 0; tb < T; tb += SX_ENS_RB) {
        float qt[SX_ENS_RB], sum[SX_ENS_RB];
#pragma unroll
        for (int i = 0; i < SX_ENS_RB; ++i) {
            const size_t o = (size_t)min(tb + i, T - 1) * SP;
            qt[i] = q[o];
            // D8 order; "+ 0" for an absent upstream cell is exact (sx_kernels.h:855-863)
            const float v0 = nup > 0 ? u0[o] : 0.f, v1 = nup > 1 ? u1[o] : 0.f;
            sum[i] = v0 + v1;
        }
        for (int c = 2; c < nup; ++c) {
            const float* uc = E.qt + (size_t)upk[c] * row + s;
#pragma unroll
            for (int i = 0; i < SX_ENS_RB; ++i) sum[i] = sum[i] + uc[(size_t)min(tb + i, T - 1) * SP];
        }
#pragma unroll
        for (int i = 0; i < SX_ENS_RB; ++i)
            if (tb + i < T) q[(size_t)(tb + i) * SP] = sx_route_step(R, sum[i], qt[i], hlr);
    }
    *hl = hlr;
}

// discharge of the gauge cells of a chunk into the gauge series of the whole period
__global__ __launch_bounds__(64) void sx_k_ens_gauges(SxEnsArrays E, int nt, int t0, int T) {
    const int s = blockIdx.x * 64 + threadIdx.x, g = blockIdx.z;
    for (int t = blockIdx.y; t < T; t += gridDim.y)
        E.qg[((size_t)g * nt + t0 + t) * E.SP + s] = E.qt[((size_t)E.gauge_k[g] * E.Tc + t) * E.SP + s];
}

// ------------------------------------------------------------------------------------------------
// cost: one thread per (gauge, sample) folds the gauge series in time order -- the reference's sequential fp32 sums, and with the
// samples on the lanes no cross-lane step (sx_k_cost_sums needs __shfl only because its lanes are time steps)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sx_k_ens_cost_gauge(SxCostArgs C, SxEnsArrays E) {
    SX_LIBM_INIT();
    const int s = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    SxGaugeSums S; S.n = 0; S.sum_x = S.sum_y = S.sum_xx = S.sum_yy = S.sum_xy = S.se = S.lg = 0.f;
    const float w = C.wgauge[g];
    if (w > 0.f || w < 0.f) {
        bool want_lg = false;
        for (int j = 0; j < C.njf; ++j) want_lg |= (C.jobs_fun[j] == 6);
        const float* y = E.qg + (size_t)g * C.nt * E.SP + s;
        for (int t = C.s0; t < C.nt; ++t) {
            const float xi = sx_qo(C, g, t);
            const float yi = y[(size_t)t * E.SP] * C.dt / C.area[g] * 1e3f;          // sx_qs
            sx_sums_add(S, xi, yi, want_lg);
        }
    }
    E.gj[(size_t)g * E.SP + s] = sx_gauge_jobs(C, S);
}

// heap_sort (mwd_cost.f90:594-673) on a strided column: the comparisons and moves of sx_heap_sort_idx without the permutation
__device__ inline void sx_heap_sort_strided(int n, float* arr, size_t st) {
    if (n < 2) return;
    int l = n / 2 + 1, ir = n;
    for (;;) {
        float arr_l;
        if (l > 1) { l = l - 1; arr_l = arr[(size_t)(l - 1) * st]; }
        else {
            arr_l = arr[(size_t)(ir - 1) * st];
            arr[(size_t)(ir - 1) * st] = arr[0];
            ir = ir - 1;
            if (ir == 1) { arr[0] = arr_l; return; }
        }
        int i = l, j = l + l;
        while (j <= ir) {
            if (j < ir && arr[(size_t)(j - 1) * st] < arr[(size_t)j * st]) j = j + 1;
            if (arr_l < arr[(size_t)(j - 1) * st]) { arr[(size_t)(i - 1) * st] = arr[(size_t)(j - 1) * st]; i = j; j = j + j; }
            else j = ir + 1;
        }
        arr[(size_t)(i - 1) * st] = arr_l;
    }
}

// one thread per sample: weighted sum over the gauges in gauge order, or the median over the negative-weight gauges
// (the forward part of sx_k_cost_final, phase 0)
__global__ __launch_bounds__(64) void sx_k_ens_cost_final(SxCostArgs C, SxEnsArrays E) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    const size_t SP = (size_t)E.SP;
    float jobs = 0.f;
    int arr_size = 0;
    float* arr = E.med + s;
    for (int g = 0; g < C.ng; ++g) {
        const float w = C.wgauge[g];
        if (!(w > 0.f || w < 0.f)) continue;
        const float gauge_jobs = E.gj[(size_t)g * SP + s];
        if (w > 0.f) jobs = jobs + w * gauge_jobs;
        else { arr[(size_t)arr_size * SP] = gauge_jobs; ++arr_size; }
    }
    if (arr_size > 0) {      // quantile(arr, 0.5) replaces the weighted sum (mwd_cost.f90:154, 675-723)
        float res = arr[0];
        if (arr_size > 1) {
            sx_heap_sort_strided(arr_size, arr, SP);
            const float frac = (float)(arr_size - 1) * 0.5f + 1.f;
            if (frac <= 1.f) res = arr[0];
            else if (frac >= (float)arr_size) res = arr[(size_t)(arr_size - 1) * SP];
            else {
                const int k = (int)frac;
                const float q1 = arr[(size_t)(k - 1) * SP], q2 = arr[(size_t)k * SP];
                res = q1 + (q2 - q1) * (frac - (float)k);
            }
        }
        jobs = res;
    }
    E.cost[s] = jobs;
}

// gauge series out: qg [g][t][sample] -> qout [sample][t][g] (res_qsim(ng, nt, S) of the batch, gauge fastest)
__global__ __launch_bounds__(64) void sx_k_ens_qsim_out(SxEnsArrays E, int ng, int nt) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    for (int t = blockIdx.y; t < nt; t += gridDim.y) {
        float* o = E.qout + ((size_t)s * nt + t) * ng;
        for (int g = 0; g < ng; ++g) o[g] = E.qg[((size_t)g * nt + t) * E.SP + s];
    }
}
