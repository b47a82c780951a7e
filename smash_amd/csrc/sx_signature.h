// sx_signature.h -- the signature-based criteria of the cost: Crc, Cfp2/10/50/90, Epf, Elt, Erc.
//
//   signature / flow_percentile / quantile / heap_sort   smash/solver/optimize/mwd_cost.f90:594-970
//   SIGNATURE_B, FLOW_PERCENTILE_B, QUANTILE_B, HEAP_SORT_B   smash/solver/forward/forward_db.f90:4132-4370, 4434-4473, 4655-4926
//   SIGNATURE_D, FLOW_PERCENTILE_D, QUANTILE_D, HEAP_SORT_D   forward_db.f90:4284-4322, 4403-4429, 4501-4650
//
// Included by sx_cost.h (after SxCostArgs, sx_qs and sx_qo), which carries only the hooks.  The criteria hold no libm call, only IEEE
// + - * / and abs, so both builds of the library form the same bits.  What is restated as written: the event loop's
// num / den carried over an Erc event that skips its assignment; event sums and maxima masked on qo >= 0 and po >= 0 only; maxima
// from 0 with a strict >, imax = 0 when nothing exceeds 0; an event's extent start .. start + count - 1 from its first occurrence;
// sequential fp32 sums in time order; the percentile's compaction on qo >= 0 and qs >= 0 and its heap sort, whose own moves decide
// which of several equal values ends at a sorted position -- the sort carries the time steps along, as sx_heap_sort_idx does for the
// median over gauges, and the adjoint seeds the steps it left at the two interpolation points.
//
// Three kernels in front of sx_k_cost_final:
//   sx_k_sig_sums   one wavefront per gauge: 64 consecutive steps loaded coalesced, folded in time order through cross-lane reads
//                   (the scheme of sx_k_cost_sums); the Crc sums over the period, then sums, maxima and argmaxima of every event
//   sx_k_sig_pct    one workgroup per gauge: wave-wide compaction in time order (ballot + prefix count) into LDS (8 B per step; a
//                   series beyond the LDS of a compute unit uses a scratch buffer of the plan); then a radix select of the two
//                   interpolation points of every Cfp*, taken when each selected value occurs once; else -- ties, or
//                   SMASHX_SIG_REPLAY=1 -- the reference's heap sort replayed with the steps carried along by one lane
//   sx_k_sig_obs    the same for the observed series, once per smashx_set_options: the denominators do not move between sweeps
// sx_k_cost_final then evaluates the criteria (sx_sig_eval), sx_k_cost_seeds adds their seeds (sx_sig_seed) and sx_k_cost_tangent their
// tangents (sx_sig_tangent).
#pragma once

#define SX_JF_CRC 7      // SMASHX_CRC ... SMASHX_ERC of include/smashx.h
#define SX_JF_CFP2 8
#define SX_JF_CFP90 11
#define SX_JF_EPF 12
#define SX_JF_ELT 13
#define SX_JF_ERC 14
#define SX_SIG_WANT_CRC 1u
#define SX_SIG_WANT_EVENTS 2u
#define SX_SIG_WANT_PCT 4u

__device__ inline void sx_heap_sort_idx(int n, float* arr, int* idx);    // sx_cost.h

// mwd_cost.f90:946-958
__device__ __forceinline__ float sx_sig_p(int q) { return q == 0 ? 0.02f : q == 1 ? 0.1f : q == 2 ? 0.5f : 0.9f; }

__device__ __forceinline__ bool sx_sig_event_kind(int fun) { return fun >= SX_JF_EPF && fun <= SX_JF_ERC; }

// ---- sums over the period (Crc) and per event (Epf, Elt, Erc) -----------------------------------------------------------------------
struct SxSigFold { float sum_qo, sum_qs, sum_po, max_qo, max_qs, max_po; int imax_qo, imax_qs, imax_po; };
// one flow percentile of a gauge: numerator, denominator, and where the numerator came from: steps k1 (weight 1 - f) and k2 (weight f),
// -1 = none
struct SxSigPct { float num, den, f; int k1, k2; };

// steps [a, a + cnt) of gauge g folded in time order; j1 = 1-based position of step a in the reference's slice (imax_* are positions
// in that slice, 0 = none).  Every lane ends with the same values.
__device__ __forceinline__ SxSigFold sx_sig_fold(const SxCostArgs& C, int g, int a, int cnt, int lane) {
    SxSigFold F; F.sum_qo = F.sum_qs = F.sum_po = F.max_qo = F.max_qs = F.max_po = 0.f; F.imax_qo = F.imax_qs = F.imax_po = 0;
    const int end = a + cnt;
    for (int tb = a; tb < end; tb += 64) {
        const int t = tb + lane;
        float x = -1.f, y = 0.f, po = -1.f;
        if (t < end) { x = sx_qo(C, g, t); y = sx_qs(C, g, t); po = C.sig.po[(size_t)g * C.nt + t]; }
        const int m = min(64, end - tb);
        for (int i = 0; i < m; ++i) {
            const float xi = __shfl(x, i), yi = __shfl(y, i), pi = __shfl(po, i);
            if (xi >= 0.f && pi >= 0.f) {
                const int j = tb + i - C.s0 + 1;
                F.sum_qo = F.sum_qo + xi;
                F.sum_qs = F.sum_qs + yi;
                F.sum_po = F.sum_po + pi;
                if (xi > F.max_qo) { F.max_qo = xi; F.imax_qo = j; }
                if (yi > F.max_qs) { F.max_qs = yi; F.imax_qs = j; }
                if (pi > F.max_po) { F.max_po = pi; F.imax_po = j; }
            }
        }
    }
    return F;
}

__global__ __launch_bounds__(64) void sx_k_sig_sums(SxCostArgs C) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const float w = C.wgauge[g];
    if (!(w > 0.f || w < 0.f)) return;
    if (C.sig.want & SX_SIG_WANT_CRC) {
        const SxSigFold F = sx_sig_fold(C, g, C.s0, C.nt - C.s0, lane);
        if (lane == 0) { C.sig.crc[g * 3 + 0] = F.sum_qo; C.sig.crc[g * 3 + 1] = F.sum_qs; C.sig.crc[g * 3 + 2] = F.sum_po; }
    }
    if (C.sig.want & SX_SIG_WANT_EVENTS) {
        const int nev = C.sig.nev[g];
        for (int i = 0; i < nev; ++i) {
            const int a = C.sig.ev[(g * C.sig.maxev + i) * 2], cnt = C.sig.ev[(g * C.sig.maxev + i) * 2 + 1];
            const SxSigFold F = sx_sig_fold(C, g, a, cnt, lane);
            if (lane == 0) C.sig.evres[g * C.sig.maxev + i] = F;
        }
    }
}

// ---- flow percentiles --------------------------------------------------------------------------------------------------------------
// the steps of [s0, nt) with qo >= 0 (and, unless obs, qs >= 0) compacted in time order: key = qo (obs) or qs, idx = the time step.
// Returns their number on every lane.
__device__ __forceinline__ int sx_sig_compact(const SxCostArgs& C, int g, bool obs, bool keys_obs, float* key, int* idx, int lane) {
    int n = 0;
    for (int tb = C.s0; tb < C.nt; tb += 64) {
        const int t = tb + lane;
        float x = -1.f, y = -1.f;
        if (t < C.nt) { x = sx_qo(C, g, t); y = obs ? 0.f : sx_qs(C, g, t); }
        const bool keep = x >= 0.f && y >= 0.f;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
            key[pos] = keys_obs ? x : y; idx[pos] = t;
        }
        n += __popcll(m);
    }
    return n;
}

// quantile (mwd_cost.f90:675-723) of a series already heap-sorted with its steps: the value, the one or two steps it reads and the
// interpolation weight.  n = 0 reads the first entry of flow_percentile's zeroed work array.
__device__ __forceinline__ void sx_sig_quantile(int n, const float* key, const int* idx, float p, float& v, int& k1, int& k2, float& f) {
    v = 0.f; k1 = -1; k2 = -1; f = 0.f;
    if (n == 0) return;
    v = key[0]; k1 = idx[0];
    if (n > 1) {
        const float frac = (float)(n - 1) * p + 1.f;
        if (frac <= 1.f) { v = key[0]; k1 = idx[0]; }
        else if (frac >= (float)n) { v = key[n - 1]; k1 = idx[n - 1]; }
        else {
            const int k = (int)frac;
            const float q1 = key[k - 1], q2 = key[k];
            f = frac - (float)k;
            v = q1 + (q2 - q1) * f;
            k1 = idx[k - 1]; k2 = idx[k];
        }
    }
}

extern __shared__ __align__(8) unsigned char sx_sig_lds[];

__device__ __forceinline__ void sx_sig_buffers(const SxCostArgs& C, int g, float*& key, int*& idx) {
    const int len = C.nt - C.s0;
    if (C.sig.lds) { key = (float*)sx_sig_lds; idx = (int*)(sx_sig_lds + (size_t)len * sizeof(float)); }
    else { key = C.sig.skey + (size_t)g * C.nt; idx = C.sig.sidx + (size_t)g * C.nt; }
}

// once per smashx_set_options: n_obs = steps with qo >= 0, den_obs = the quantiles of those
__global__ __launch_bounds__(64) void sx_k_sig_obs(SxCostArgs C) {
    const int g = blockIdx.x, lane = threadIdx.x;
    float* key; int* idx; sx_sig_buffers(C, g, key, idx);
    const int n = sx_sig_compact(C, g, true, true, key, idx, lane);
    __syncthreads();
    if (lane != 0) return;
    sx_heap_sort_idx(n, key, idx);
    C.sig.n_obs[g] = n;
    for (int q = 0; q < 4; ++q) {
        float v, f; int k1, k2;
        sx_sig_quantile(n, key, idx, sx_sig_p(q), v, k1, k2, f);
        C.sig.den_obs[g * 4 + q] = v;
    }
}

// The values at sorted positions r of the compacted series WITHOUT sorting it: a radix select over the bit patterns (keys are >= 0, so
// they order like unsigned integers), 8 bits a pass, the whole workgroup counting into 256 LDS bins.  The last pass leaves the
// multiplicity of the selected value: the fast path is taken only when every selected value occurs exactly once, because then the time
// step it came from is the one the heap sort would leave there; with equal values the sort's own moves decide and it is replayed.
#define SX_SIG_PCT_THREADS 256
struct SxSigSelect { unsigned hist[256]; unsigned prefix, rank, count; int n, bad, step; };

__device__ __forceinline__ void sx_sig_select(SxSigSelect& S, int n, const float* key, const int* idx, unsigned r, int tid,
                                              float& value, int& step, unsigned& count) {
    unsigned mask = 0u;
    if (tid == 0) { S.prefix = 0u; S.rank = r; S.step = -1; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        S.hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = S.prefix;
        for (int i = tid; i < n; i += SX_SIG_PCT_THREADS) {
            const unsigned u = __float_as_uint(key[i]);
            if ((u & mask) == prefix) atomicAdd(&S.hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned c = 0u, rank = S.rank; int b = 0;
            for (; b < 255; ++b) { if (rank < c + S.hist[b]) break; c += S.hist[b]; }
            S.rank = rank - c; S.prefix = prefix | ((unsigned)b << shift); S.count = S.hist[b];
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned bits = S.prefix;
    for (int i = tid; i < n; i += SX_SIG_PCT_THREADS)
        if (__float_as_uint(key[i]) == bits) S.step = idx[i];            // (one writer when count == 1; else the caller replays)
    __syncthreads();
    value = __uint_as_float(bits); step = S.step; count = S.count;
    __syncthreads();
}

__global__ __launch_bounds__(SX_SIG_PCT_THREADS) void sx_k_sig_pct(SxCostArgs C) {
    __shared__ SxSigSelect S;
    __shared__ SxSigPct P4[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    const float w = C.wgauge[g];
    if (!(w > 0.f || w < 0.f)) return;
    float* key; int* idx; sx_sig_buffers(C, g, key, idx);
    if (tid < 64) { const int m = sx_sig_compact(C, g, false, false, key, idx, tid); if (tid == 0) { S.n = m; S.bad = 0; } }
    __syncthreads();
    const int n = S.n;
    const bool same_obs = n == C.sig.n_obs[g];
    bool fast = !C.sig.replay && same_obs && n >= 2;
    if (fast) {
        for (int i = tid; i < n; i += SX_SIG_PCT_THREADS) if (__float_as_uint(key[i]) == 0x80000000u) S.bad = 1;     // -0 orders as +0
        __syncthreads();
        for (int q = 0; q < 4 && !S.bad; ++q) {
            const float frac = (float)(n - 1) * sx_sig_p(q) + 1.f;
            SxSigPct P; P.f = 0.f; P.k2 = -1; P.den = C.sig.den_obs[g * 4 + q];
            float v1, v2 = 0.f; int s1, s2 = -1; unsigned c1, c2 = 1u;
            if (frac <= 1.f) sx_sig_select(S, n, key, idx, 0u, tid, v1, s1, c1);
            else if (frac >= (float)n) sx_sig_select(S, n, key, idx, (unsigned)(n - 1), tid, v1, s1, c1);
            else {
                const int k = (int)frac;
                sx_sig_select(S, n, key, idx, (unsigned)(k - 1), tid, v1, s1, c1);
                sx_sig_select(S, n, key, idx, (unsigned)k, tid, v2, s2, c2);
                P.f = frac - (float)k;
            }
            if (c1 != 1u || c2 != 1u) { if (tid == 0) S.bad = 1; }
            else if (tid == 0) {
                P.k1 = s1;
                if (s2 >= 0) { P.num = v1 + (v2 - v1) * P.f; P.k2 = s2; } else P.num = v1;
                P4[q] = P;
            }
            __syncthreads();
        }
        fast = !S.bad;
        if (fast) { if (tid < 4) C.sig.pct[g * 4 + tid] = P4[tid]; return; }
    }
    // the replay: the reference's heap sort with the steps carried along, one lane
    if (tid == 0) {
        sx_heap_sort_idx(n, key, idx);
        for (int q = 0; q < 4; ++q) {
            SxSigPct P;
            sx_sig_quantile(n, key, idx, sx_sig_p(q), P.num, P.k1, P.k2, P.f);
            P.den = C.sig.den_obs[g * 4 + q];
            C.sig.pct[g * 4 + q] = P;
        }
    }
    if (same_obs) return;
    // a step with qo >= 0 whose qs is negative or NaN left the compaction: the observed series loses it too (mwd_cost.f90:755)
    __syncthreads();
    if (tid < 64) sx_sig_compact(C, g, false, true, key, idx, tid);
    __syncthreads();
    if (tid != 0) return;
    sx_heap_sort_idx(n, key, idx);
    for (int q = 0; q < 4; ++q) {
        float v, f; int k1, k2;
        sx_sig_quantile(n, key, idx, sx_sig_p(q), v, k1, k2, f);
        C.sig.pct[g * 4 + q].den = v;
    }
}

// ---- the criteria from what the kernels above left (single thread of sx_k_cost_final) -------------------------------------------------
// num / den of event i for criterion fun, the reference's SELECT CASE (mwd_cost.f90:878-899); false: Erc skipped its assignment
__device__ __forceinline__ bool sx_sig_event_numden(int fun, const SxSigFold& E, float& num, float& den) {
    if (fun == SX_JF_EPF) { num = E.max_qs; den = E.max_qo; return true; }
    if (fun == SX_JF_ELT) { num = (float)(E.imax_qs - E.imax_po); den = (float)(E.imax_qo - E.imax_po); return true; }
    if (E.sum_po > 0.f) { num = E.sum_qs / E.sum_po; den = E.sum_qo / E.sum_po; return true; }
    return false;
}

// signature (mwd_cost.f90:772-970) of criterion j at gauge g; with c != nullptr also SIGNATURE_B for the seed res_b: the coefficients
// sx_sig_seed reads (per event in C.sig.evcoef).  num / den start at 0: smashx_set_options refuses every input on which the reference
// would read them unassigned.
__device__ inline float sx_sig_eval(const SxCostArgs& C, int g, int j, float res_b, SxCostCoef* c) {
    const int fun = C.jobs_fun[j];
    float res = 0.f, num = 0.f, den = 0.f;
    if (sx_sig_event_kind(fun)) {
        const int nev = C.sig.nev[g];
        for (int i = 0; i < nev; ++i) {
            const SxSigFold E = C.sig.evres[g * C.sig.maxev + i];
            const bool assigned = sx_sig_event_numden(fun, E, num, den);
            int flag = 0;
            if (den > 0.f) { const float x = num / den - 1.f; res = res + fabsf(x); flag = (x >= 0.f) ? 1 : 2; }
            if (c) { C.sig.evden[i] = den; C.sig.evflag[i] = flag | (assigned ? 4 : 0); }
        }
        if (nev > 0) res = res / (float)nev;
        if (c) {
            float rb = res_b;
            if (nev > 0) rb = rb / (float)nev;
            float num_b = 0.f;
            for (int i = nev - 1; i >= 0; --i) {
                const int flag = C.sig.evflag[i];
                if ((flag & 3) == 1) num_b = num_b + rb / C.sig.evden[i];
                else if ((flag & 3) == 2) num_b = num_b - rb / C.sig.evden[i];
                float coef = 0.f;
                if (fun == SX_JF_EPF) { coef = num_b; num_b = 0.f; }
                else if (fun == SX_JF_ELT) num_b = 0.f;
                else if (flag & 4) { coef = num_b / C.sig.evres[g * C.sig.maxev + i].sum_po; num_b = 0.f; }
                C.sig.evcoef[((size_t)g * SX_MAXJF + j) * C.sig.maxev + i] = coef;
            }
            c->kind = fun == SX_JF_ERC ? 6 : fun == SX_JF_EPF ? 7 : 0;
        }
        return res;
    }
    float sum_po = 0.f, f = 0.f; int k1 = -1, k2 = -1;
    if (fun == SX_JF_CRC) {
        sum_po = C.sig.crc[g * 3 + 2];
        if (sum_po > 0.f) { num = C.sig.crc[g * 3 + 1] / sum_po; den = C.sig.crc[g * 3 + 0] / sum_po; }
    } else {
        const SxSigPct P = C.sig.pct[g * 4 + (fun - SX_JF_CFP2)];
        num = P.num; den = P.den; f = P.f; k1 = P.k1; k2 = P.k2;
    }
    float num_b = 0.f;
    if (den > 0.f) {
        const float x = num / den - 1.f;
        res = fabsf(x);
        num_b = (x >= 0.f) ? res_b / den : -(res_b / den);
    }
    if (c) {
        if (fun == SX_JF_CRC) { c->kind = 5; c->c = (sum_po > 0.f) ? num_b / sum_po : 0.f; }
        else { c->kind = 8; c->c = num_b; c->c_xy = f; c->i0 = k1; c->i1 = k2; }
    }
    return res;
}

// what criterion j adds to qs_b(t) of gauge g, in the reference's order of accumulation: events last to first
__device__ __forceinline__ float sx_sig_seed(const SxCostArgs& C, int g, int j, int t, float x, const SxCostCoef& c, float y_b) {
    if (c.kind == 8) {
        // QUANTILE_B: q2_b = temp_b, q1_b = res_b - temp_b (forward_db.f90:4353-4359); HEAP_SORT_B only moves them back to their steps
        const float temp_b = c.c_xy * c.c;
        if (t == c.i1) y_b = y_b + temp_b;
        if (t == c.i0) y_b = y_b + (c.c - temp_b);
        return y_b;
    }
    const float po = C.sig.po[(size_t)g * C.nt + t];
    const bool masked = x >= 0.f && po >= 0.f;
    if (c.kind == 5) { if (masked) y_b = y_b + c.c; return y_b; }
    const int nev = C.sig.nev[g];
    for (int i = nev - 1; i >= 0; --i) {
        const float coef = C.sig.evcoef[((size_t)g * SX_MAXJF + j) * C.sig.maxev + i];
        if (c.kind == 6) {
            const int a = C.sig.ev[(g * C.sig.maxev + i) * 2], cnt = C.sig.ev[(g * C.sig.maxev + i) * 2 + 1];
            if (masked && t >= a && t < a + cnt) y_b = y_b + coef;
        } else {
            const int im = C.sig.evres[g * C.sig.maxev + i].imax_qs;
            if (im > 0 && t == C.s0 + im - 1) y_b = y_b + coef;
        }
    }
    return y_b;
}

// SIGNATURE_D (forward_db.f90:4501-4650) of criterion j at gauge g: returns the value, res_d its tangent along yd (q_d at the gauge
// cell, scaled like COMPUTE_JOBS_D scales qs_d).  One thread, sequential in time like the rest of sx_k_cost_tangent; maxima, argmaxima
// and the percentiles' steps are those the value pass (sx_k_sig_sums / sx_k_sig_pct) left.
__device__ inline float sx_sig_tangent(const SxCostArgs& C, int g, int j, const float* yd, float& res_d) {
    const int fun = C.jobs_fun[j];
    const float sc = C.dt * 1e3f;
    const float ar = C.area[g];
    float res = 0.f, num = 0.f, den = 0.f, num_d = 0.f;
    res_d = 0.f;
    if (sx_sig_event_kind(fun)) {
        const int nev = C.sig.nev[g];
        for (int i = 0; i < nev; ++i) {
            const SxSigFold E = C.sig.evres[g * C.sig.maxev + i];
            if (fun == SX_JF_EPF) {
                num_d = (E.imax_qs > 0) ? sc * yd[C.s0 + E.imax_qs - 1] / ar : 0.f;
                num = E.max_qs; den = E.max_qo;
            } else if (fun == SX_JF_ELT) {
                num = (float)(E.imax_qs - E.imax_po); den = (float)(E.imax_qo - E.imax_po); num_d = 0.f;
            } else if (E.sum_po > 0.f) {
                const int a = C.sig.ev[(g * C.sig.maxev + i) * 2], cnt = C.sig.ev[(g * C.sig.maxev + i) * 2 + 1];
                float sum_qs_d = 0.f;
                for (int t = a; t < a + cnt; ++t)
                    if (sx_qo(C, g, t) >= 0.f && C.sig.po[(size_t)g * C.nt + t] >= 0.f) sum_qs_d = sum_qs_d + sc * yd[t] / ar;
                num_d = sum_qs_d / E.sum_po; num = E.sum_qs / E.sum_po; den = E.sum_qo / E.sum_po;
            }
            if (den > 0.f) {
                const float x = num / den - 1.f;
                if (x >= 0.f) { res_d = res_d + num_d / den; res = res + x; }
                else { res_d = res_d + (-(num_d / den)); res = res + (-x); }
            }
        }
        if (nev > 0) { res_d = res_d / (float)nev; res = res / (float)nev; }
        return res;
    }
    if (fun == SX_JF_CRC) {
        const float sum_po = C.sig.crc[g * 3 + 2];
        if (sum_po > 0.f) {
            float sum_qs_d = 0.f;
            for (int t = C.s0; t < C.nt; ++t)
                if (sx_qo(C, g, t) >= 0.f && C.sig.po[(size_t)g * C.nt + t] >= 0.f) sum_qs_d = sum_qs_d + sc * yd[t] / ar;
            num_d = sum_qs_d / sum_po; num = C.sig.crc[g * 3 + 1] / sum_po; den = C.sig.crc[g * 3 + 0] / sum_po;
        }
    } else {
        const SxSigPct P = C.sig.pct[g * 4 + (fun - SX_JF_CFP2)];
        num = P.num; den = P.den;
        if (P.k2 >= 0) { const float q1_d = sc * yd[P.k1] / ar, q2_d = sc * yd[P.k2] / ar; num_d = q1_d + P.f * (q2_d - q1_d); }
        else if (P.k1 >= 0) num_d = sc * yd[P.k1] / ar;
    }
    if (den > 0.f) {
        const float x = num / den - 1.f;
        if (x >= 0.f) { res_d = num_d / den; res = x; }
        else { res_d = -(num_d / den); res = -x; }
    }
    return res;
}
