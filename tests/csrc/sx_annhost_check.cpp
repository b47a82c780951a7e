// sx_annhost_check.cpp -- the plain-C++ host side of the ANN regionalisation (smash_amd/csrc/sx_annhost.h over sx_ann.h: the graph's
// checks and normal form, the device limits, the network's forward pass and weight gradient) on a masked grid, every buffer a heap
// block of exactly the size the library's caller owes: built with -fsanitize=address,undefined -ffp-contract=off by
// tests/test_ann_host_sanitized.py.  argv: nrow ncol nd.  Prints "ok <active cells> <weights>" or "VIOLATION ...".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../smash_amd/csrc/sx_annhost.h"
#include "../../smash_amd/csrc/sx_hyperhost.h"

#define FAIL(msg) do { puts("VIOLATION " msg); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int nrow = atoi(argv[1]), ncol = atoi(argv[2]), nd = atoi(argv[3]);
    const size_t n2 = (size_t)nrow * ncol;
    const char* why = nullptr;
    SxAnnNet N{};
    // ---- the graph's checks ----
    const int ncv = 3;
    const double lower[ncv] = {1.0, -20.0, 0.5}, upper[ncv] = {900.0, 5.0, 0.75};
    {
        std::unique_ptr<int[]> kind(new int[8]{SMASHX_ANN_DENSE, SMASHX_ANN_ELU, SMASHX_ANN_DENSE, SMASHX_ANN_TANH, SMASHX_ANN_LEAKY_RELU,
                                               SMASHX_ANN_DENSE, SMASHX_ANN_SIGMOID, SMASHX_ANN_SCALE});
        std::unique_ptr<int[]> width(new int[8]{5, 5, 4, 4, 4, ncv, ncv, ncv});
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, lower, upper, &N, &why)) FAIL("a good graph refused");
        if (N.nstage != 3 || N.nw != (nd + 1) * 5 + 6 * 4 + 5 * ncv || N.nslots != nd + 5 + 4 + ncv + 5 || N.soff != nd + 12) FAIL("normal form");
        if (N.st[1].ne != 2 || N.st[2].e0 != 3 || N.st[2].woff != (nd + 1) * 5 + 24 || sx_annh_device_refusal(N)) FAIL("stages");
        SxAnnNet M{};
        if (sx_annh_build(0, 8, kind.get(), width.get(), ncv, lower, upper, &M, &why) != SMASHX_E_ARG) FAIL("nd = 0 passes");
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv + 1, lower, upper, &M, &why) != SMASHX_E_ARG) FAIL("a wrong last width passes");
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, nullptr, upper, &M, &why) != SMASHX_E_ARG) FAIL("a scale layer without bounds passes");
        if (sx_annh_build(nd, 7, kind.get() + 1, width.get() + 1, ncv, lower, upper, &M, &why) != SMASHX_E_ARG) FAIL("a first layer that is not dense passes");
        width[1] = 6;
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, lower, upper, &M, &why) != SMASHX_E_ARG) FAIL("an element-wise width passes");
        width[1] = 5;
        for (int k : {SMASHX_ANN_SOFTPLUS, SMASHX_ANN_SOFTMAX, SMASHX_ANN_DROPOUT}) {
            kind[1] = k;
            if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, lower, upper, &M, &why) != SMASHX_E_UNSUPPORTED) FAIL("a refused layer kind passes");
        }
        kind[1] = 0;
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, lower, upper, &M, &why) != SMASHX_E_ARG) FAIL("kind 0 passes");
        kind[1] = SMASHX_ANN_ELU;
        width[0] = width[1] = 65;         // the host takes it, the device does not
        if (sx_annh_build(nd, 8, kind.get(), width.get(), ncv, lower, upper, &M, &why) || !sx_annh_device_refusal(M)) FAIL("a wide layer");
        std::unique_ptr<int[]> k5(new int[5]{1, 1, 1, 1, 1}), w5(new int[5]{4, 4, 4, 4, ncv});
        if (sx_annh_build(nd, 5, k5.get(), w5.get(), ncv, nullptr, nullptr, &M, &why) || !sx_annh_device_refusal(M)) FAIL("five dense layers");
        std::unique_ptr<int[]> k33(new int[33]), w33(new int[33]);
        for (int i = 0; i < 33; ++i) { k33[i] = i ? SMASHX_ANN_RELU : SMASHX_ANN_DENSE; w33[i] = ncv; }
        if (sx_annh_build(nd, 33, k33.get(), w33.get(), ncv, nullptr, nullptr, &M, &why) != SMASHX_E_UNSUPPORTED) FAIL("33 layers pass");
        std::unique_ptr<int[]> k1(new int[1]{SMASHX_ANN_DENSE}), w25(new int[1]{25});
        if (sx_annh_build(nd, 1, k1.get(), w25.get(), 25, nullptr, nullptr, &M, &why) != SMASHX_E_UNSUPPORTED) FAIL("25 outputs pass");
        // the LDS rows of the device: (64, 64, 64, 24) on 32 inputs is exactly 312, one more input is refused; the host takes both
        std::unique_ptr<int[]> k4(new int[4]{1, 1, 1, 1}), w4(new int[4]{64, 64, 64, 24});
        if (sx_annh_build(32, 4, k4.get(), w4.get(), 24, nullptr, nullptr, &M, &why) || M.nslots != SX_ANN_DEV_SLOTS || sx_annh_device_refusal(M)) FAIL("312 rows refused");
        if (sx_annh_build(33, 4, k4.get(), w4.get(), 24, nullptr, nullptr, &M, &why) || M.nslots != SX_ANN_DEV_SLOTS + 1 || !sx_annh_device_refusal(M)) FAIL("313 rows pass");
    }
    // ---- a ragged mask, the plan's cells in an order of its own (reversed stripes); the descriptors gathered and put in position order ----
    std::vector<int> cell_flat;
    for (int c = ncol - 1; c >= 0; --c)
        for (int r = 0; r < nrow; ++r)
            if ((r * 7 + c * 3) % 5 != 1) cell_flat.push_back(r + c * nrow);
    const size_t n = cell_flat.size();
    std::unique_ptr<float[]> desc(new float[(size_t)nd * n2]);
    for (size_t i = 0; i < (size_t)nd * n2; ++i) desc[i] = (float)((i * 37 % 101) / 100.0);
    std::vector<float> g;
    sx_hh_gather(desc.get(), nd, n2, cell_flat, g);
    const std::vector<int> order = sx_hh_order(cell_flat);
    std::unique_ptr<float[]> x(new float[n * nd + (n == 0)]), lg(new float[n * ncv + (n == 0)]), y(new float[n * ncv + (n == 0)]);
    for (size_t c = 0; c < n; ++c) {
        for (int i = 0; i < nd; ++i) x[c * nd + i] = g[(size_t)i * n + order[c]];
        for (int j = 0; j < ncv; ++j) lg[c * ncv + j] = (float)(((c * 13 + j * 7) % 23) - 11) * 0.125f;
    }
    std::unique_ptr<double[]> w(new double[N.nw]), wb(new double[N.nw]);
    for (int i = 0; i < N.nw; ++i) w[i] = ((i * 29 % 41) - 20) / 16.0;
    sx_annh_forward(N, w.get(), n, x.get(), (size_t)nd, 1, y.get());
    for (size_t c = 0; c < n; ++c)
        for (int j = 0; j < ncv; ++j) {
            const float v = y[c * ncv + j];
            if (!(v >= (float)lower[j] && v <= (float)upper[j])) FAIL("an output outside the scale layer's bounds");
        }
    sx_annh_gradient(N, w.get(), n, x.get(), (size_t)nd, 1, lg.get(), wb.get());
    bool any = false;
    for (int i = 0; i < N.nw; ++i) { if (!std::isfinite(wb[i])) FAIL("a gradient that is not finite"); any = any || wb[i] != 0.0; }
    if (n > 0 && !any) FAIL("a zero gradient");
    for (size_t i = 0; i < n * ncv; ++i) lg[i] = 0.f;
    sx_annh_gradient(N, w.get(), n, x.get(), (size_t)nd, 1, lg.get(), wb.get());
    for (int i = 0; i < N.nw; ++i) if (wb[i] != 0.0) FAIL("a zero loss_grad leaves a gradient");
    // ---- one dense layer and nothing else: grad_W = X^T G and grad_b = sum G in the stated order, block by block, exactly ----
    {
        std::unique_ptr<int[]> kind(new int[1]{SMASHX_ANN_DENSE}), width(new int[1]{ncv});
        SxAnnNet L{};
        if (sx_annh_build(nd, 1, kind.get(), width.get(), ncv, nullptr, nullptr, &L, &why) || L.nw != (nd + 1) * ncv) FAIL("the linear net");
        for (size_t i = 0; i < n * ncv; ++i) lg[i] = (float)((i * 11 % 19) - 9) * 0.25f;
        std::unique_ptr<double[]> lw(new double[L.nw]), lb(new double[L.nw]);
        for (int i = 0; i < L.nw; ++i) lw[i] = 0.5 - i * 0.03125;
        sx_annh_gradient(L, lw.get(), n, x.get(), (size_t)nd, 1, lg.get(), lb.get());
        for (int c = 0; c < L.nw; ++c) {
            double total = 0.0;
            for (size_t c0 = 0; c0 < n; c0 += SX_ANN_BLOCK) {
                double part = 0.0;
                for (size_t k = c0; k < n && k < c0 + SX_ANN_BLOCK; ++k) {
                    if (c < nd * ncv) part = part + (double)x[k * nd + c / ncv] * (double)lg[k * ncv + c % ncv];
                    else part = part + (double)lg[k * ncv + (c - nd * ncv)];
                }
                total = total + part;
            }
            if (lb[c] != total) FAIL("the order of the weight-gradient sums");
        }
    }
    printf("ok %zu %d\n", n, N.nw);
    return 0;
}
