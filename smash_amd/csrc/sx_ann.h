// sx_ann.h -- the arithmetic contract of the ANN regionalisation (include/smashx_ann.h): the network of the reference's
// smash/core/net.py as far as the descriptor -> parameter mapping uses it, written once for the host (sx_annhost.h) and the device
// (sx_annmap.h), which therefore compute the same fp64 bits.
//
// Storage and precision: fp32 descriptors in (normalised by the caller), fp64 inside, each output rounded to nearest once into an fp32
// field; the fp32 cell gradients of the adjoint sweep come in as loss_grad and are widened exactly.
//
// Layers (net.py:579-842): dense x.W + b with W (fin, fout) row-major and b (fout) -- packed per dense layer W, then b --; the
// activations relu, leaky_relu (0.2), elu (0.1), selu, sigmoid and tanh = 2 / (1 + exp(-2x)) - 1 by the reference's formulas; scale
// lower + x (upper - lower).  A graph is normalised to STAGES: one dense layer and the element-wise layers (activation, scale) behind
// it.  softplus, softmax and dropout are not part of the contract.
//
// Bit rule: every product and sum goes through SX_ANN_MUL / SX_ANN_ADD -- __dmul_rn / __dadd_rn on the device, plain operators on the
// host, which is built with contraction off (-ffp-contract=off) --, divisions are IEEE, and exp is sx_ann_exp below on both sides, so
// that no libm takes part.  A dot product starts from the bias and adds the products in ascending input index; the back-propagated
// delta of input i starts from the product of output 0 and adds in ascending output index.
//
// Order of the weight-gradient sums grad_W = X^T.G, grad_b = sum G over the active cells: the cells are taken in column-major position
// (sx_hh_order), in BLOCKS of SX_ANN_BLOCK = 64 consecutive positions (the last one shorter).  A block's partial starts at +0 and adds
// its cells' terms in ascending position; the total starts at +0 and adds the block partials in ascending block order.  The
// association depends on the number of active cells alone.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SX_ANN_HD __host__ __device__ inline
#else
#define SX_ANN_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SX_ANN_MUL(a, b) __dmul_rn((a), (b))
#define SX_ANN_ADD(a, b) __dadd_rn((a), (b))
#else
#define SX_ANN_MUL(a, b) ((a) * (b))
#define SX_ANN_ADD(a, b) ((a) + (b))
#endif
#define SX_ANN_SUB(a, b) SX_ANN_ADD((a), -(b))

// layer kinds: the values of the enum of include/smashx_ann.h (sx_annhost.h asserts the equality)
#define SX_ANN_DENSE 1
#define SX_ANN_RELU 2
#define SX_ANN_LEAKY_RELU 3
#define SX_ANN_ELU 4
#define SX_ANN_SELU 5
#define SX_ANN_SIGMOID 6
#define SX_ANN_TANH 7
#define SX_ANN_SCALE 8

#define SX_ANN_BLOCK 64        // positions per block of the weight-gradient sums: a constant of the format
#define SX_ANN_MAXL 32         // layers of a graph
#define SX_ANN_MAXCV 24        // outputs: one per model field at most
// what the kernels take (the host path takes any width): dense layers, width of a dense layer, LDS slots of 64 doubles
#define SX_ANN_DEV_DENSE 4
#define SX_ANN_DEV_WIDTH 64
#define SX_ANN_DEV_SLOTS 312   // 156 KiB of the 160 KiB of a compute unit

struct SxAnnStage {
    int fin, fout;             // the dense layer
    int woff;                  // W at weights[woff], b at weights[woff + fin * fout]
    int zoff;                  // slot of its outputs
    int e0, ne;                // the element-wise layers behind it: ekind[e0 .. e0 + ne)
};
struct SxAnnNet {
    int nd, ncv, nstage, nw;   // inputs, outputs, stages, packed weights
    int nslots;                // nd + sum of the widths + the widest: inputs, every stage's outputs, one scratch row
    int soff;                  // slot of the scratch row
    SxAnnStage st[SX_ANN_MAXL];
    int ekind[SX_ANN_MAXL];
    double lower[SX_ANN_MAXCV], upper[SX_ANN_MAXCV];       // of the scale layer
};

// ---- exp ----------------------------------------------------------------------------------------------------------------------------------
// x = k ln2 + r with k = x / ln2 rounded to nearest (by the 1.5 * 2^52 addition) and ln2 split in two (the high part has 21 trailing
// zero bits, so k * hi is exact), |r| <= 0.3466 (1 + 1e-9); exp(r) = 1 + (r + r^2 P(r)) with the Taylor coefficients 1/2! .. 1/13!
// (truncation 0.3466^14 / 14! = 4e-18); the result is scaled by 2^k in one exact multiplication, or two where 2^k is no normal number.
// Plain IEEE multiplications and additions, the same on both sides.  NaN -> NaN, +inf -> +inf, -inf -> +0, overflow above
// 709.782712893384 -> +inf, below -745.2 -> +0.
SX_ANN_HD double sx_ann_pow2(int k) {         // 2^k, -1022 <= k <= 1023
    const uint64_t u = (uint64_t)(k + 1023) << 52;
    double d;
    memcpy(&d, &u, 8);
    return d;
}
SX_ANN_HD double sx_ann_exp(double x) {
    if (x != x) return SX_ANN_ADD(x, x);
    if (x > 709.782712893384) return sx_ann_pow2(1023) * 2.0;
    if (x < -745.2) return 0.0;
    const double shift = 6755399441055744.0;       // 1.5 * 2^52
    const double kd = SX_ANN_SUB(SX_ANN_ADD(SX_ANN_MUL(x, 1.44269504088896338700e+00), shift), shift);
    const int k = (int)kd;
    double r = SX_ANN_SUB(x, SX_ANN_MUL(kd, 6.93147180369123816490e-01));
    r = SX_ANN_SUB(r, SX_ANN_MUL(kd, 1.90821492927058770002e-10));
    double p = 1.0 / 6227020800.0;
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 479001600.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 39916800.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 3628800.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 362880.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 40320.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 5040.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 720.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 120.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 24.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 1.0 / 6.0);
    p = SX_ANN_ADD(SX_ANN_MUL(p, r), 0.5);
    const double e = SX_ANN_ADD(1.0, SX_ANN_ADD(r, SX_ANN_MUL(SX_ANN_MUL(r, r), p)));
    if (k > 1023) return SX_ANN_MUL(SX_ANN_MUL(e, sx_ann_pow2(k - 1)), 2.0);
    if (k < -1022) return SX_ANN_MUL(SX_ANN_MUL(e, sx_ann_pow2(k + 1000)), sx_ann_pow2(-1000));
    return SX_ANN_MUL(e, sx_ann_pow2(k));
}

// ---- element-wise layers: value and derivative at input x; j is the neuron (the scale layer's bounds) -----------------------------------------
#define SX_ANN_SELU_ALPHA 1.6732632423543772848170429916717
#define SX_ANN_SELU_SCALE 1.0507009873554804934193349852946
SX_ANN_HD double sx_ann_value(const SxAnnNet& N, int kind, int j, double x) {
    switch (kind) {
    case SX_ANN_RELU: return x >= 0.0 ? x : 0.0;
    case SX_ANN_LEAKY_RELU: return x >= 0.0 ? x : SX_ANN_MUL(0.2, x);
    case SX_ANN_ELU: return x >= 0.0 ? x : SX_ANN_MUL(0.1, SX_ANN_SUB(sx_ann_exp(x), 1.0));
    case SX_ANN_SELU: return SX_ANN_MUL(SX_ANN_SELU_SCALE, x >= 0.0 ? x : SX_ANN_MUL(SX_ANN_SELU_ALPHA, SX_ANN_SUB(sx_ann_exp(x), 1.0)));
    case SX_ANN_SIGMOID: return 1.0 / SX_ANN_ADD(1.0, sx_ann_exp(-x));
    case SX_ANN_TANH: return SX_ANN_SUB(2.0 / SX_ANN_ADD(1.0, sx_ann_exp(SX_ANN_MUL(-2.0, x))), 1.0);
    case SX_ANN_SCALE: return SX_ANN_ADD(N.lower[j], SX_ANN_MUL(x, SX_ANN_SUB(N.upper[j], N.lower[j])));
    }
    return x;
}
SX_ANN_HD double sx_ann_slope(const SxAnnNet& N, int kind, int j, double x) {
    switch (kind) {
    case SX_ANN_RELU: return x >= 0.0 ? 1.0 : 0.0;
    case SX_ANN_LEAKY_RELU: return x >= 0.0 ? 1.0 : 0.2;
    case SX_ANN_ELU: return x >= 0.0 ? 1.0 : SX_ANN_ADD(sx_ann_value(N, SX_ANN_ELU, j, x), 0.1);
    case SX_ANN_SELU: return SX_ANN_MUL(SX_ANN_SELU_SCALE, x >= 0.0 ? 1.0 : SX_ANN_MUL(SX_ANN_SELU_ALPHA, sx_ann_exp(x)));
    case SX_ANN_SIGMOID: { const double s = sx_ann_value(N, SX_ANN_SIGMOID, j, x); return SX_ANN_MUL(s, SX_ANN_SUB(1.0, s)); }
    case SX_ANN_TANH: { const double t = sx_ann_value(N, SX_ANN_TANH, j, x); return SX_ANN_SUB(1.0, SX_ANN_MUL(t, t)); }
    case SX_ANN_SCALE: return SX_ANN_SUB(N.upper[j], N.lower[j]);
    }
    return 1.0;
}
// neuron j of stage t: its output behind the first m element-wise layers, given its dense output z
SX_ANN_HD double sx_ann_chain(const SxAnnNet& N, int t, int j, double z, int m) {
    for (int q = 0; q < m; ++q) z = sx_ann_value(N, N.ekind[N.st[t].e0 + q], j, z);
    return z;
}
// ... and the gradient g of its output taken back to z, layer by layer from the last one, each at the input it saw
SX_ANN_HD double sx_ann_chain_b(const SxAnnNet& N, int t, int j, double z, double g) {
    for (int q = N.st[t].ne - 1; q >= 0; --q)
        g = SX_ANN_MUL(g, sx_ann_slope(N, N.ekind[N.st[t].e0 + q], j, sx_ann_chain(N, t, j, z, q)));
    return g;
}

// ---- one cell.  S(i) is slot i of the cell: a double& (the host keeps a cell's slots [slot][cell of the block] as the device keeps them in
// LDS, so the two run the same text).  Slots 0 .. nd - 1 hold the inputs. --------------------------------------------------------------------
// the inputs of stage t into the scratch row: the previous stage's outputs behind its element-wise layers
template <class Slots>
SX_ANN_HD void sx_ann_stage_inputs(const SxAnnNet& N, int t, Slots S) {
    const SxAnnStage& P = N.st[t - 1];
    for (int i = 0; i < P.fout; ++i) S(N.soff + i) = sx_ann_chain(N, t - 1, i, S(P.zoff + i), P.ne);
}
// the forward pass: every stage's dense outputs into its slots
template <class Slots>
SX_ANN_HD void sx_ann_forward(const SxAnnNet& N, const double* __restrict__ w, Slots S) {
    for (int t = 0; t < N.nstage; ++t) {
        const SxAnnStage& T = N.st[t];
        if (t > 0) sx_ann_stage_inputs(N, t, S);
        const int in = t > 0 ? N.soff : 0;
        const double* W = w + T.woff;
        const double* b = W + (size_t)T.fin * T.fout;
        for (int j = 0; j < T.fout; ++j) {
            double z = b[j];
            for (int i = 0; i < T.fin; ++i) z = SX_ANN_ADD(z, SX_ANN_MUL(S(in + i), W[(size_t)i * T.fout + j]));
            S(T.zoff + j) = z;
        }
    }
}
// output j of the network after sx_ann_forward, rounded once
template <class Slots>
SX_ANN_HD float sx_ann_output(const SxAnnNet& N, int j, Slots S) {
    const int t = N.nstage - 1;
    return (float)sx_ann_chain(N, t, j, S(N.st[t].zoff + j), N.st[t].ne);
}
// the last stage's slots from dense outputs to their deltas, given the gradient of output j in G(j)
template <class Slots, class Grad>
SX_ANN_HD void sx_ann_seed(const SxAnnNet& N, Slots S, Grad G) {
    const int t = N.nstage - 1;
    for (int j = 0; j < N.st[t].fout; ++j) S(N.st[t].zoff + j) = sx_ann_chain_b(N, t, j, S(N.st[t].zoff + j), G(j));
}
// stage t's deltas back through its weights and the element-wise layers of stage t - 1, whose slots turn from dense outputs to deltas
template <class Slots>
SX_ANN_HD void sx_ann_back(const SxAnnNet& N, const double* __restrict__ w, int t, Slots S) {
    const SxAnnStage &T = N.st[t], &P = N.st[t - 1];
    const double* W = w + T.woff;
    for (int i = 0; i < T.fin; ++i) {
        double g = SX_ANN_MUL(S(T.zoff), W[(size_t)i * T.fout]);
        for (int j = 1; j < T.fout; ++j) g = SX_ANN_ADD(g, SX_ANN_MUL(S(T.zoff + j), W[(size_t)i * T.fout + j]));
        S(P.zoff + i) = sx_ann_chain_b(N, t - 1, i, S(P.zoff + i), g);
    }
}
// chain c of stage t -- entry c of its packed (W, b) -- over the nc cells of a block: B(slot, cell) is slot `slot` of cell `cell`, the
// stage's inputs lie in the row `in` (the scratch row, or row 0 for the first stage), its deltas in its own slots
template <class Block>
SX_ANN_HD double sx_ann_partial(const SxAnnNet& N, int t, int c, int nc, Block B) {
    const SxAnnStage& T = N.st[t];
    const int in = t > 0 ? N.soff : 0;
    double s = 0.0;
    if (c < T.fin * T.fout) {
        const int i = c / T.fout, j = c - i * T.fout;
        for (int k = 0; k < nc; ++k) s = SX_ANN_ADD(s, SX_ANN_MUL(B(in + i, k), B(T.zoff + j, k)));
    } else {
        const int j = c - T.fin * T.fout;
        for (int k = 0; k < nc; ++k) s = SX_ANN_ADD(s, B(T.zoff + j, k));
    }
    return s;
}
