// sx_tablehost.h -- the host tables of the sample paths and the forcing statistics (smashx.hip uploads them) in plain C++17: the river
// forest of smashx_multiple_run / smashx_uniform_costs, the per-thread tables of the catchment-resident kernel (sx_resident.h), the
// catchment lists of smashx_mean_forcing and the index lists of smashx_prcp_indices (sx_prcpindices.h).  No device pointer and no HIP
// call: a CPU program can include this file (tests/csrc/sx_tablehost_check.cpp runs it under AddressSanitizer +
// UndefinedBehaviorSanitizer).  The upstream order is the reference's summation order and the list order its column-major sum: what
// is built here decides results bit for bit.  Compile with -ffp-contract=off: every fp32 operation below is rounded on its own.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "sx_plan.h"
#include "sx_tables.h"

// f(i, fn) for every neighbour of flat cell c that drains into it, in ascending D8 code i + 1; fn its flat index.  flwdir_grid: the
// D8 codes of EVERY cell of the grid, active or not (0 = none)
template <class F> inline void sx_th_drains_in(const SxSchedule& s, const signed char* flwdir_grid, long c, F f) {
    const int nrow = s.nrow, ncol = s.ncol, row = (int)(c % nrow), col = (int)(c / nrow);
    for (int i = 0; i < 8; ++i) {
        const long fn = sx_d8_upstream(nrow, ncol, row, col, i);
        if (fn >= 0 && flwdir_grid[fn] == i + 1) f(i, fn);
    }
}

// ---- the river forest over the plan's cells ----------------------------------------------------------------------------------------
struct SxForest {
    int n = 0, nlevels = 0;
    std::vector<int> up, upn;        // [n][8], [n]: the plan cells draining into cell k, in ascending D8 code; unused entries -1
    std::vector<int> parent;         // [n]: the cell k drains into, -1 for a root
    std::vector<int> level;          // [n]: the longest path from a leaf (a leaf: 0)
    std::vector<int> order;          // [n]: cells by level, ascending plan index inside a level
    std::vector<int> level_begin;    // [nlevels + 1]: level l is order[level_begin[l] .. level_begin[l + 1])
};
// k_of_flat >= 0 means "active and in this plan", so the codes of the whole grid serve.  A cycle: *error set, the forest is not usable
inline SxForest sx_forest(const SxSchedule& s, const signed char* flwdir_grid, std::string* error) {
    SxForest F;
    const int n = F.n = s.n;
    F.up.assign((size_t)n * 8, -1); F.upn.assign(n, 0); F.parent.assign(n, -1); F.level.assign(n, 0);
    for (int k = 0; k < n; ++k)
        sx_th_drains_in(s, flwdir_grid, s.cell_flat[k], [&](int, long fn) {
            const int ku = s.k_of_flat[fn];
            if (ku >= 0) { F.up[(size_t)k * 8 + F.upn[k]++] = ku; F.parent[ku] = k; }
        });
    std::vector<int> indeg(F.upn), topo; topo.reserve(n);
    for (int k = 0; k < n; ++k) if (indeg[k] == 0) topo.push_back(k);
    for (size_t i = 0; i < topo.size(); ++i) {
        const int k = topo[i], q = F.parent[k];
        if (q >= 0) { F.level[q] = std::max(F.level[q], F.level[k] + 1); if (--indeg[q] == 0) topo.push_back(q); }
    }
    if ((int)topo.size() != n) { *error = "flow directions contain a cycle over active cells"; return F; }
    for (int k = 0; k < n; ++k) F.nlevels = std::max(F.nlevels, F.level[k] + 1);
    F.order.resize(n); F.level_begin.assign(F.nlevels + 1, 0);
    for (int k = 0; k < n; ++k) F.level_begin[F.level[k] + 1]++;
    for (int l = 0; l < F.nlevels; ++l) F.level_begin[l + 1] += F.level_begin[l];
    std::vector<int> fill(F.level_begin.begin(), F.level_begin.end() - 1);
    for (int k = 0; k < n; ++k) F.order[fill[F.level[k]]++] = k;
    return F;
}

// ---- the per-thread tables of sx_k_res_fwd (SxResTables), thread i = cell order[i] ---------------------------------------------------
struct SxResHost {
    std::vector<int> cell, level, upline, upn, ownline, gfirst, gnext;
    size_t floats = 0;               // of all delay lines together
    std::string refusal;             // not empty: the catchment is beyond the kernel's limits, the tables are not usable
};
inline std::string sx_res_cells_refusal(int n) {
    return std::to_string(n) + " active cells, the resident kernel holds one cell per thread and at most " + std::to_string(SX_RES_MAXCELLS);
}
// lds_limit_bytes: what a workgroup may claim; static_bytes: what the kernel holds statically (the exact-libm build's tables)
inline SxResHost sx_res_host_tables(const SxForest& F, const std::vector<int>& gauge_k, int ng, size_t lds_limit_bytes, size_t static_bytes) {
    SxResHost R;
    const int n = F.n;
    if (n > SX_RES_MAXCELLS) { R.refusal = sx_res_cells_refusal(n); return R; }
    std::vector<int> pos(n);
    for (int i = 0; i < n; ++i) pos[F.order[i]] = i;
    R.cell = F.order; R.level.resize(n); R.upn.resize(n); R.ownline.assign(n, -1);
    R.upline.assign((size_t)n * 8, 0); R.gfirst.assign(n, -1); R.gnext.assign(std::max(ng, 1), -1);
    size_t floats = 0;
    for (int i = 0; i < n; ++i) {          // lines in thread order: neighbours in a level are neighbours in LDS
        const int k = F.order[i];
        R.level[i] = F.level[k]; R.upn[i] = F.upn[k];
        if (F.parent[k] < 0) continue;
        const int D = F.level[F.parent[k]] - F.level[k];         // >= 1
        int lg = 1;
        while ((1 << lg) < D + 1) ++lg;                          // D + 1 slots, rounded up to a power of two (sx_resident.h)
        if (floats + ((size_t)1 << lg) > ((size_t)1 << 26)) { floats = (size_t)1 << 26; break; }
        R.ownline[i] = (int)(floats << 5) | lg;
        floats += (size_t)1 << lg;
    }
    if (floats * 4 + static_bytes > lds_limit_bytes) {
        R.refusal = "the delay lines of the catchment need " + (floats >= ((size_t)1 << 26) ? std::string("more than 268435456") : std::to_string(floats * 4 + static_bytes)) +
                    " B of LDS, a workgroup may claim " + std::to_string(lds_limit_bytes);
        return R;
    }
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < R.upn[i]; ++c) R.upline[(size_t)i * 8 + c] = R.ownline[pos[F.up[(size_t)R.cell[i] * 8 + c]]];
    for (int g = ng - 1; g >= 0; --g) {      // gauges of a cell chained in gauge order
        const int k = gauge_k[g];
        if (k < 0 || k >= n) continue;
        R.gnext[g] = R.gfirst[pos[k]]; R.gfirst[pos[k]] = g;
    }
    R.floats = floats;
    return R;
}

// ---- the catchments of the gauges ----------------------------------------------------------------------------------------------------
// mask_upstream_cells (mw_mask.f90:11-54) restated without recursion: from the gauge cell, every neighbour whose D8 code points at a
// cell already taken is taken, over the whole grid; the mask read in flat order (row + col * nrow) IS the column-major order of the
// reference's sums.
struct SxCatchments {
    std::vector<int> count;          // ng: cells of the catchment
    std::vector<int> begin;          // ng + 1: its list in `list`, padded with -1 to whole blocks of 64 entries
    std::vector<int> list;           // plan cells
};
inline SxCatchments sx_catchment_lists(const SxSchedule& s, const signed char* flwdir_grid, int ng, std::string* refusal) {
    SxCatchments C;
    const long n2 = (long)s.nrow * s.ncol;
    std::vector<char> mask((size_t)n2); std::vector<long> stack;
    C.begin.assign(1, 0);
    for (int g = 0; g < ng; ++g) {
        std::fill(mask.begin(), mask.end(), 0);
        const long c0 = s.cell_flat[s.gauge_k[g]];
        mask[c0] = 1; stack.assign(1, c0);
        while (!stack.empty()) {
            const long c = stack.back(); stack.pop_back();
            sx_th_drains_in(s, flwdir_grid, c, [&](int, long fn) { if (!mask[fn]) { mask[fn] = 1; stack.push_back(fn); } });
        }
        for (long c = 0; c < n2; ++c) {
            if (!mask[c]) continue;
            const int k = s.k_of_flat[c];
            if (k < 0) {
                *refusal = "smashx_mean_forcing: the catchment of gauge " + std::to_string(g) + " contains the inactive cell (" + std::to_string(c % s.nrow) + ", " +
                           std::to_string(c / s.nrow) + "): the plan holds no forcing there";
                return C;
            }
            C.list.push_back(k);
        }
        C.count.push_back((int)C.list.size() - C.begin[g]);
        while (C.list.size() % 64) C.list.push_back(-1);
        if (C.list.size() > (size_t)INT_MAX - 64) { *refusal = "smashx_mean_forcing: the catchment lists of all gauges together exceed 2^31 entries"; return C; }
        C.begin.push_back((int)C.list.size());
    }
    return C;
}

// ---- the lists and constants of compute_prcp_indices (mw_forcing_statistic.f90:77-220) ------------------------------------------------
// Per gauge, as the reference does it once per call: d = flwdst - flwdst(gauge) over the WHOLE grid in fp32; the catchment with its d
// and d * d; flwdst_qtl = quantile1d_r (m_statistic.f90:231-277) of the catchment's d at q = real(i) / 100, i = 0, 10 .. 100; wf, the
// cumulated counts of the catchment's d per bin; the ten bins (qtl(k-1) < d <= qtl(k)) over the whole grid, column-major inside a bin;
// the cell (gauge_row, gauge_row), which the reference reads for pwf(1) (:181 indexes the column with the gauge's row: reproduced as
// written).  Whatever the reference would read and the plan holds no forcing for is refused.
struct SxPiHost {
    std::vector<int> list;           // per gauge the catchment and the ten bins, every section padded with -1 to whole blocks of 64
    std::vector<float> dl, d2l;      // d and d * d of the catchment entries, padded with 0
    std::vector<SxPiGauge> gauges;
    long entries = 0, catchment_entries = 0;
};
// quantile1d_r for the eleven quantiles; b sorted, at least 2 values
inline void sx_pi_quantiles(const std::vector<float>& b, float* qtl) {
    const int n = (int)b.size();
    for (int i = 0; i < SX_PI_NQ; ++i) {
        const float q = (float)(10 * i) / 100.f;
        if (q >= 1.f) { qtl[i] = b[n - 1]; continue; }
        const float div = q * (float)(n - 1) + 1.f;
        const int qt = (int)floorf(div);
        const float r = fmodf(div, (float)qt);
        qtl[i] = (1.f - r) * b[qt - 1] + r * b[qt];
    }
}
inline SxPiHost sx_pi_host_tables(const SxSchedule& s, const SxCatchments& C, const float* flwdst, int ng, std::string* refusal) {
    SxPiHost P;
    const int nrow = s.nrow, ncol = s.ncol;
    const long n2 = (long)nrow * ncol;
    auto refuse = [&](const std::string& why) { *refusal = "smashx_prcp_indices: " + why; return P; };
    std::vector<float> d((size_t)n2), b; std::vector<int> bins[SX_PI_NQ];
    std::vector<int>& list = P.list;
    P.gauges.resize((size_t)ng);
    for (int g = 0; g < ng; ++g) {
        SxPiGauge& G = P.gauges[g];
        const long c0 = s.cell_flat[s.gauge_k[g]];
        const int row = (int)(c0 % nrow);
        const float f0 = flwdst[c0];
        for (long c = 0; c < n2; ++c) d[c] = flwdst[c] - f0;
        const int nc = C.count[g];
        if (nc < 2) return refuse("the catchment of gauge " + std::to_string(g) + " has " + std::to_string(nc) + " cell: the reference's quantile reads two");
        const int krr = row < ncol ? s.k_of_flat[row + (long)row * nrow] : -1;
        if (krr < 0)
            return refuse("gauge " + std::to_string(g) + ": the reference reads the rain of the cell (gauge_row, gauge_row) = (" + std::to_string(row) + ", " +
                          std::to_string(row) + "), which is " + (row < ncol ? "inactive: the plan holds no forcing there" : "outside the grid"));
        G.krr = krr; G.lb = (int)list.size(); G.db = (int)P.dl.size();
        b.clear();
        for (int j = 0; j < nc; ++j) {
            const int k = C.list[(size_t)C.begin[g] + j];
            const float dc = d[s.cell_flat[k]];
            list.push_back(k); P.dl.push_back(dc); P.d2l.push_back(dc * dc); b.push_back(dc);
        }
        while (list.size() % 64) { list.push_back(-1); P.dl.push_back(0.f); P.d2l.push_back(0.f); }
        P.catchment_entries += nc;
        G.sec[0] = 0; G.sec[1] = (int)((list.size() - (size_t)G.lb) / 64);
        std::sort(b.begin(), b.end());
        float qtl[SX_PI_NQ];
        sx_pi_quantiles(b, qtl);
        G.wf[0] = 1.f; G.cnt[0] = 0.f;
        for (int k = 1; k < SX_PI_NQ; ++k) {
            int cnt = 0;
            for (float v : b) cnt += (v > qtl[k - 1] && v <= qtl[k]) ? 1 : 0;
            G.wf[k] = G.wf[k - 1] + (float)cnt;
            bins[k].clear();
        }
        for (long c = 0; c < n2; ++c) {                        // flat order is the column-major order of the reference's sums
            for (int k = 1; k < SX_PI_NQ; ++k) {
                if (!(d[c] > qtl[k - 1] && d[c] <= qtl[k])) continue;
                const int kk = s.k_of_flat[c];
                if (kk < 0)
                    return refuse("the inactive cell (" + std::to_string(c % nrow) + ", " + std::to_string(c / nrow) + ") lies in distance bin " + std::to_string(k) +
                                  " of gauge " + std::to_string(g) + ": the plan holds no forcing there");
                bins[k].push_back(kk);
            }
        }
        for (int k = 1; k < SX_PI_NQ; ++k) {
            list.insert(list.end(), bins[k].begin(), bins[k].end());
            while (list.size() % 64) list.push_back(-1);
            G.cnt[k] = (float)bins[k].size();
            G.sec[k + 1] = (int)((list.size() - (size_t)G.lb) / 64);
        }
        if (list.size() > (size_t)INT_MAX - 64) return refuse("the lists of all gauges together exceed 2^31 entries");
    }
    P.entries = (long)list.size();
    return P;
}
