// sx_hyperhost.h -- the host side of the hyper maps on the device (smashx_hyper_*, smashx.hip) that is plain C++17: the argument checks,
// the gather of the descriptors to plan-cell order, the order of the adjoint's sums, the closing of the gradient matrices and the
// scatter of a cell vector into a caller's plane.  No device pointer and no HIP call: a CPU program can include this file alone
// (tests/csrc/sx_hyperhost_check.cpp runs it under AddressSanitizer + UndefinedBehaviorSanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <numeric>
#include <vector>

#include "sx_fields.h"

// 0: fine; else the reason smashx_hyper_set_descriptors returns SMASHX_E_ARG with
inline const char* sx_hh_bad_arguments(int mapping, int nd) {
    if (mapping != SMASHX_HYPER_LINEAR && mapping != SMASHX_HYPER_POLYNOMIAL) return "mapping: SMASHX_HYPER_LINEAR or SMASHX_HYPER_POLYNOMIAL expected";
    if (nd < 0) return "nd < 0";
    return nullptr;
}
inline int sx_hh_nhyper(int mapping, int nd) { return mapping == SMASHX_HYPER_POLYNOMIAL ? 1 + 2 * nd : 1 + nd; }

// descriptor (nrow, ncol, nd) column-major, n2 = nrow * ncol -> out[j * n + k] = descriptor j at plan cell k
inline void sx_hh_gather(const float* descriptor, int nd, size_t n2, const std::vector<int>& cell_flat, std::vector<float>& out) {
    const size_t n = cell_flat.size();
    out.resize((size_t)nd * n);
    for (int j = 0; j < nd; ++j)
        for (size_t k = 0; k < n; ++k) out[(size_t)j * n + k] = descriptor[(size_t)j * n2 + (size_t)cell_flat[k]];
}
// the plan cells in ascending flat index row + col * nrow: column index outer, row index inner -- the order of the reference's sums
inline std::vector<int> sx_hh_order(const std::vector<int>& cell_flat) {
    std::vector<int> order(cell_flat.size());
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return cell_flat[a] < cell_flat[b]; });
    return order;
}
// sums[e * nh + r], e over the nf fields field[e] of the launch -> the two gradient matrices (nh, 16) / (nh, 8), both overwritten:
// HYPER_*_B adds every sum to a zeroed entry, the columns of the other fields stay zero
inline void sx_hh_close(const float* sums, const int* field, int nf, int nh, float* hyper_parameters_b, float* hyper_states_b) {
    std::memset(hyper_parameters_b, 0, (size_t)nh * SMASHX_GNP * sizeof(float));
    std::memset(hyper_states_b, 0, (size_t)nh * SMASHX_GNS * sizeof(float));
    for (int e = 0; e < nf; ++e) {
        const int f = field[e];
        float* col = sx_field_is_state(f) ? hyper_states_b + (size_t)(f - SMASHX_GNP) * nh : hyper_parameters_b + (size_t)f * nh;
        for (int r = 0; r < nh; ++r) col[r] = 0.f + sums[(size_t)e * nh + r];
    }
}
// a cell vector into the active cells of a caller's (nrow, ncol) plane; every other cell keeps its value
inline void sx_hh_scatter(const float* cellv, const std::vector<int>& cell_flat, float* plane) {
    for (size_t k = 0; k < cell_flat.size(); ++k) plane[cell_flat[k]] = cellv[k];
}
