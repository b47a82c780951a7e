// sx_annmap.h -- the network of the ANN regionalisation on the device (include/smashx_ann.h): the arithmetic is sx_ann.h,
// the same text the host runs (sx_annhost.h), so planes and weight gradients equal the host's bit for bit.
//
// One wavefront per workgroup, one cell per lane.  A cell's slots -- its inputs, every stage's dense outputs (which the adjoint turns
// into the stage's deltas in place) and one scratch row for a stage's inputs -- lie in LDS as [slot][lane]: a dynamically indexed
// per-lane array would go to scratch memory, and consecutive lanes hit consecutive 8-byte words this way.  The LDS of a workgroup is
// nslots * 512 B, sized at launch from the graph (156 KiB at the device limits, one wavefront per compute unit; 44 KiB for a
// (32, 16, 4) net on 4 descriptors, 3 workgroups).  The weights are wave-uniform: every lane reads the same address, straight from
// HBM / L2 through the read-only path.
//   sx_k_ann_map     the forward pass at plan cell k into the control fields' cell vectors and planes (the triple of SxHmFields)
//   sx_k_ann_terms   the adjoint's parallel part, one workgroup per BLOCK of 64 positions of a span: forward pass, the cell gradients
//                    of the sweep taken back to the deltas, and per stage -- last to first -- the block's partial of every weight
//                    chain, one LANE per chain walking the block's cells in ascending position, into terms[block of the span][weight]
//   sx_k_ann_walk    the ordered part, one lane per weight: down the span's blocks, one addition per block
// The totals travel between the spans in sums[weight].  SMASHX_ANN_SPAN in the environment forces the span (cells, rounded up to whole
// blocks); the default keeps the staging rows at SX_ANN_STAGE_BYTES.
#pragma once

#include "sx_ann.h"
#include "sx_hypermap.h"       // SxHmFields: where a field's values go and where its gradient lies

#define SX_ANN_STAGE_BYTES ((size_t)32 << 20)

struct SxAnnLds { double* p; __device__ double& operator()(int i) const { return p[i * SX_ANN_BLOCK]; } };
struct SxAnnLdsBlock { const double* p; __device__ double operator()(int i, int k) const { return p[i * SX_ANN_BLOCK + k]; } };

// grid = ceil(n / 64), block = 64, dynamic LDS = N.nslots * 512.  desc[i * n + k]; flat: k -> row + col * nrow
__global__ __launch_bounds__(SX_ANN_BLOCK)
void sx_k_ann_map(SxAnnNet N, SxHmFields F, const double* __restrict__ w, const float* __restrict__ desc, const int* __restrict__ flat, int n) {
    extern __shared__ double sx_ann_slots[];
    const int k = blockIdx.x * SX_ANN_BLOCK + threadIdx.x;
    if (k >= n) return;                     // (no barrier below: a lane touches its own column only)
    const SxAnnLds S{sx_ann_slots + threadIdx.x};
    for (int i = 0; i < N.nd; ++i) S(i) = (double)desc[(size_t)i * n + k];
    sx_ann_forward(N, w, S);
    for (int e = 0; e < N.ncv; ++e) {
        const float v = sx_ann_output(N, e, S);
        F.val[e][k] = v;
        if (F.start[e]) F.start[e][k] = v;
        if (F.full[e]) F.full[e][flat[k]] = v;
    }
}

// grid = ceil(ns / 64), block = 64, dynamic LDS = N.nslots * 512.  order: position among the active cells in column-major order ->
// plan cell; the span is positions [c0, c0 + ns), c0 a multiple of 64; terms: [block of the span][N.nw]
__global__ __launch_bounds__(SX_ANN_BLOCK)
void sx_k_ann_terms(SxAnnNet N, SxHmFields F, const double* __restrict__ w, const float* __restrict__ desc, const int* __restrict__ order,
                    int n, int c0, int ns, double* __restrict__ terms) {
    extern __shared__ double sx_ann_slots[];
    const int lane = threadIdx.x;
    const int nc = min(SX_ANN_BLOCK, ns - (int)blockIdx.x * SX_ANN_BLOCK);       // cells of this block: uniform
    const bool cell = lane < nc;
    const SxAnnLds S{sx_ann_slots + lane};
    if (cell) {
        const int k = order[c0 + blockIdx.x * SX_ANN_BLOCK + lane];
        for (int i = 0; i < N.nd; ++i) S(i) = (double)desc[(size_t)i * n + k];
        sx_ann_forward(N, w, S);
        sx_ann_seed(N, S, [&](int e) { return F.grad[e] ? (double)F.grad[e][k] : 0.0; });      // a field nothing reads: zero
    }
    __syncthreads();
    const SxAnnLdsBlock B{sx_ann_slots};
    double* out = terms + (size_t)blockIdx.x * N.nw;
    for (int t = N.nstage - 1; t >= 0; --t) {
        if (t > 0) {
            if (cell) sx_ann_stage_inputs(N, t, S);
            __syncthreads();
        }
        const int nchain = (N.st[t].fin + 1) * N.st[t].fout;
        for (int c = lane; c < nchain; c += SX_ANN_BLOCK) out[N.st[t].woff + c] = sx_ann_partial(N, t, c, nc, B);
        if (t > 0) {
            __syncthreads();
            if (cell) sx_ann_back(N, w, t, S);
            __syncthreads();
        }
    }
}

// grid = ceil(nw / 64), block = 64: lane = weight.  sums[weight] carries the total from span to span (zeroed before the first)
__global__ __launch_bounds__(64)
void sx_k_ann_walk(const double* __restrict__ terms, int nblocks, int nw, double* __restrict__ sums) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nw) return;
    double s = sums[c];
    const double* p = terms + c;
#pragma unroll 8
    for (int b = 0; b < nblocks; ++b) s = __dadd_rn(s, p[(size_t)b * nw]);      // a block's load does not depend on the running total
    sums[c] = s;
}
