// sx_annhost.h -- the host side of the ANN regionalisation (include/smashx_ann.h) that is plain C++17: the graph's checks and its
// normal form (SxAnnNet, sx_ann.h), the device limits, and the network itself on the host -- forward pass and weight gradient, the
// arithmetic of sx_ann.h in the order sx_ann.h states, so the same fp64 bits as the kernels of sx_annmap.h.  Build with contraction
// off (-ffp-contract=off).  No device pointer and no HIP call: a CPU program can include this file alone
// (tests/csrc/sx_annhost_check.cpp runs it under AddressSanitizer + UndefinedBehaviorSanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "../../include/smashx.h"
#include "sx_ann.h"

static_assert(SX_ANN_DENSE == SMASHX_ANN_DENSE && SX_ANN_RELU == SMASHX_ANN_RELU && SX_ANN_LEAKY_RELU == SMASHX_ANN_LEAKY_RELU &&
              SX_ANN_ELU == SMASHX_ANN_ELU && SX_ANN_SELU == SMASHX_ANN_SELU && SX_ANN_SIGMOID == SMASHX_ANN_SIGMOID &&
              SX_ANN_TANH == SMASHX_ANN_TANH && SX_ANN_SCALE == SMASHX_ANN_SCALE, "sx_ann.h numbers the layers like smashx_ann.h");

// The graph into its normal form.  width[l] is the output width of layer l (an element-wise layer repeats its input's).  0, or the
// error code with *why set: SMASHX_E_ARG for a graph that is none, SMASHX_E_UNSUPPORTED for the layer kinds outside the contract and a
// graph beyond the format (SX_ANN_MAXL layers, SX_ANN_MAXCV outputs).
inline int sx_annh_build(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper,
                         SxAnnNet* out, const char** why) {
    SxAnnNet N{};
    if (!kind || !width || !out) { *why = "null argument"; return SMASHX_E_ARG; }
    if (nd < 1) { *why = "nd < 1"; return SMASHX_E_ARG; }
    if (nlayers < 1 || ncv < 1) { *why = "no layers or no outputs"; return SMASHX_E_ARG; }
    for (int l = 0; l < nlayers; ++l) {
        if (kind[l] == SMASHX_ANN_SOFTPLUS || kind[l] == SMASHX_ANN_SOFTMAX || kind[l] == SMASHX_ANN_DROPOUT) {
            *why = "softplus, softmax and dropout layers are outside the contract (sx_ann.h)"; return SMASHX_E_UNSUPPORTED;
        }
        if (kind[l] < SMASHX_ANN_DENSE || kind[l] > SMASHX_ANN_DROPOUT) { *why = "layer kind: a SMASHX_ANN_* value expected"; return SMASHX_E_ARG; }
    }
    if (kind[0] != SMASHX_ANN_DENSE) { *why = "the first layer must be a dense layer"; return SMASHX_E_ARG; }
    if (nlayers > SX_ANN_MAXL || ncv > SX_ANN_MAXCV) { *why = "more layers or outputs than the format holds"; return SMASHX_E_UNSUPPORTED; }
    N.nd = nd; N.ncv = ncv;
    int w = nd, ne = 0, wmax = 0, slots = nd;
    for (int l = 0; l < nlayers; ++l) {
        if (width[l] < 1) { *why = "a layer of width < 1"; return SMASHX_E_ARG; }
        if (kind[l] == SMASHX_ANN_DENSE) {
            SxAnnStage& T = N.st[N.nstage++];
            T.fin = w; T.fout = width[l]; T.woff = N.nw; T.zoff = slots; T.e0 = ne; T.ne = 0;
            N.nw += (T.fin + 1) * T.fout;
            slots += T.fout;
            wmax = std::max(wmax, T.fout);
            w = T.fout;
        } else {
            if (width[l] != w) { *why = "an element-wise layer whose width differs from its input's"; return SMASHX_E_ARG; }
            if (kind[l] == SMASHX_ANN_SCALE) {
                if (w != ncv) { *why = "a scale layer on a width that is not ncv"; return SMASHX_E_ARG; }
                if (!lower || !upper) { *why = "a scale layer without bounds"; return SMASHX_E_ARG; }
            }
            N.ekind[ne++] = kind[l];
            N.st[N.nstage - 1].ne++;
        }
    }
    if (w != ncv) { *why = "the last layer's width is not ncv"; return SMASHX_E_ARG; }
    for (int j = 0; j < ncv; ++j) { N.lower[j] = lower ? lower[j] : 0.0; N.upper[j] = upper ? upper[j] : 1.0; }
    N.soff = slots;
    N.nslots = slots + wmax;
    *out = N;
    return 0;
}
// 0: the kernels take it; else why smashx_ann_set_net returns SMASHX_E_UNSUPPORTED
inline const char* sx_annh_device_refusal(const SxAnnNet& N) {
    if (N.nstage > SX_ANN_DEV_DENSE) return "more than 4 dense layers";
    for (int t = 0; t < N.nstage; ++t) if (N.st[t].fout > SX_ANN_DEV_WIDTH) return "a dense layer wider than 64";
    if (N.nslots > SX_ANN_DEV_SLOTS) return "nd + the sum of the dense widths + the widest exceeds the 312 rows of 64 doubles a compute unit's LDS holds";
    return nullptr;
}

// slot i of one cell / of cell k of a block, rows of SX_ANN_BLOCK doubles: the layout of the kernels' LDS
struct SxAnnhSlots { double* p; double& operator()(int i) const { return p[(size_t)i * SX_ANN_BLOCK]; } };
struct SxAnnhBlock { double* p; double operator()(int i, int k) const { return p[(size_t)i * SX_ANN_BLOCK + k]; } };

// y[cell * ncv + j] <- output j at cell; x(i, cell) = x[cell * xc + i * xi]
inline void sx_annh_forward(const SxAnnNet& N, const double* w, size_t n, const float* x, size_t xc, size_t xi, float* y) {
    std::vector<double> buf((size_t)N.nslots * SX_ANN_BLOCK);
    const SxAnnhSlots S{buf.data()};
    for (size_t c = 0; c < n; ++c) {
        for (int i = 0; i < N.nd; ++i) S(i) = (double)x[c * xc + (size_t)i * xi];
        sx_ann_forward(N, w, S);
        for (int j = 0; j < N.ncv; ++j) y[c * N.ncv + j] = sx_ann_output(N, j, S);
    }
}
// wb[nw] <- the gradient w.r.t. the packed weights given loss_grad[cell * ncv + j], the cells in the order of the sums (sx_ann.h)
inline void sx_annh_gradient(const SxAnnNet& N, const double* w, size_t n, const float* x, size_t xc, size_t xi, const float* loss_grad,
                             double* wb) {
    std::vector<double> buf((size_t)N.nslots * SX_ANN_BLOCK), part((size_t)N.nw);
    for (int c = 0; c < N.nw; ++c) wb[c] = 0.0;
    for (size_t c0 = 0; c0 < n; c0 += SX_ANN_BLOCK) {
        const int nc = (int)std::min<size_t>(SX_ANN_BLOCK, n - c0);
        for (int k = 0; k < nc; ++k) {
            const SxAnnhSlots S{buf.data() + k};
            const float* g = loss_grad + (c0 + k) * N.ncv;
            for (int i = 0; i < N.nd; ++i) S(i) = (double)x[(c0 + k) * xc + (size_t)i * xi];
            sx_ann_forward(N, w, S);
            sx_ann_seed(N, S, [g](int j) { return (double)g[j]; });
        }
        const SxAnnhBlock B{buf.data()};
        for (int t = N.nstage - 1; t >= 0; --t) {
            if (t > 0) for (int k = 0; k < nc; ++k) sx_ann_stage_inputs(N, t, SxAnnhSlots{buf.data() + k});
            const int nchain = (N.st[t].fin + 1) * N.st[t].fout;
            for (int c = 0; c < nchain; ++c) part[(size_t)N.st[t].woff + c] = sx_ann_partial(N, t, c, nc, B);
            if (t > 0) for (int k = 0; k < nc; ++k) sx_ann_back(N, w, t, SxAnnhSlots{buf.data() + k});
        }
        for (int c = 0; c < N.nw; ++c) wb[c] = wb[c] + part[c];
    }
}
