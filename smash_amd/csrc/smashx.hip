// smashx.hip -- C ABI implementation (include/smashx.h): plan, HBM residency, sweep orchestration.
// gfx950 only.  No CPU compute path: every entry point that needs the device fails without one.
#include "../../include/smashx.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: the functions are resolved at run time (rccl() below)

#include <dlfcn.h>

#include <algorithm>
#include <functional>
#include <numeric>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sx_cost.h"
#include "sx_jreg.h"
#include "sx_kernels.h"
#include "sx_ensemble.h"
#include "sx_resident.h"
#include "sx_fields.h"
#include "sx_interception.h"
#include "sx_meanforcing.h"
#include "sx_prcpindices.h"
#include "sx_hypermap.h"
#include "sx_hyperhost.h"
#include "sx_annmap.h"
#include "sx_annhost.h"
#include "sx_samplehost.h"
#include "sx_tablehost.h"
#include "sx_plan.h"
#include "sx_selftest.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(SMASHX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

// ---- small elementwise kernels on full (nrow*ncol) fields and on the cell vectors -------------------
__global__ void k_denormalize(float* a, long n, float lb, float ub) {   // mwd_parameters_manipulation.f90:199
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = a[i] * (ub - lb) + lb;
}
__global__ void k_normalize(float* a, long n, float lb, float ub) {     // mwd_parameters_manipulation.f90:172
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (a[i] - lb) / (ub - lb);
}
__global__ void k_gather(float* dst, const float* src, const int* idx, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = src[idx[k]];
}
__global__ void k_gather_rows(float* dst, const float* src, const int* idx, int n, int npad, long plane, int rows) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (k < n && r < rows) dst[(size_t)r * npad + k] = src[(size_t)r * plane + idx[k]];
}
__global__ void k_scatter(float* dst, const float* src, const int* idx, int n, float scale, int scaled) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[idx[k]] = scaled ? scale * src[k] : src[k];
}

// ---- compact forcing: encode + verify (smashx_set_forcing_layout) ---------------------------------------------
// src: fp32 rows, row r = time step t0 + r, cell k at src[r * ld + (idx ? idx[k] : k)].  A value is accepted only if the kernels'
// decode reproduces its bits; status[0] counts rejects, status[1] holds the bits of the one gap value (0 = none seen yet).
__global__ void k_encode_prcp(unsigned short* dst, const float* src, const int* idx, int n, int npad, long ld, int rows, float c,
                              unsigned* status) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (k >= n || r >= rows) return;
    const float v = src[(size_t)r * ld + (idx ? idx[k] : k)];
    unsigned code = 65535u;
    if (v < 0.f) {
        const unsigned bits = __float_as_uint(v);
        const unsigned old = atomicCAS(status + 1, 0u, bits);
        if (old != 0u && old != bits) atomicAdd(status, 1u);             // a second kind of negative value: not representable
    } else {
        const float kf = rintf(v / c);
        code = (kf >= 0.f && kf < 65535.f) ? (unsigned)kf : 65535u;
        if (code == 65535u || __float_as_uint((float)code * c) != __float_as_uint(v)) atomicAdd(status, 1u);
    }
    dst[(size_t)r * npad + k] = (unsigned short)code;
}
// one thread per (cell, day touched by the block): finds the daily value D with D * ratio(h) == pet bit for bit for every hour
// of the day inside the block (or D < 0 == every hour: a gap day); a day already set by an earlier block is only verified.
// petd holds NaN while a day is undetermined (only night hours seen so far).
__global__ void k_encode_pet(float* petd, const float* src, const int* idx, int n, int npad, long ld, int t0, int rows, int hour0,
                             const float* ratio, unsigned* status) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int d0 = (t0 + hour0) / 24, d = d0 + blockIdx.y;
    if (k >= n) return;
    const int ta = max(t0, d * 24 - hour0), tb = min(t0 + rows, (d + 1) * 24 - hour0);     // steps of day d in this block
    if (ta >= tb) return;
    const size_t col = idx ? idx[k] : k;
    float* slot = petd + (size_t)d * npad + k;
    float D = *slot;
    // two "not determined yet" marks: nothing seen (all ones) / only night hours seen, all of them +0 (then the day cannot be a gap day)
    const unsigned PENDING_ZEROS = 0x7fc00001u;
    const bool zeros_seen = __float_as_uint(D) == PENDING_ZEROS;
    auto fits = [&](float Dc) {
        for (int t = ta; t < tb; ++t) {
            const float v = src[(size_t)(t - t0) * ld + col];
            const float w = Dc < 0.f ? Dc : Dc * ratio[(t + hour0) % 24];
            if (__float_as_uint(w) != __float_as_uint(v)) return false;
        }
        return true;
    };
    if (D == D) { if (!fits(D)) atomicAdd(status, 1u); return; }
    // the hour with the largest share pins D to within two ulps; a negative value must be the whole day's
    int tbest = -1; float rbest = 0.f;
    bool allzero = true;
    for (int t = ta; t < tb; ++t) {
        const float v = src[(size_t)(t - t0) * ld + col], r = ratio[(t + hour0) % 24];
        if (__float_as_uint(v) != 0u) allzero = false;
        if (v < 0.f) { if (!zeros_seen && fits(v)) *slot = v; else atomicAdd(status, 1u); return; }   // a gap day is -99 at EVERY hour
        if (r > rbest) { rbest = r; tbest = t; }
    }
    if (tbest < 0) {                                                          // night hours only: any D >= 0 fits, stays open
        if (!allzero) atomicAdd(status, 1u); else *slot = __uint_as_float(PENDING_ZEROS);
        return;
    }
    const float v = src[(size_t)(tbest - t0) * ld + col];
    const unsigned b0 = __float_as_uint(v / rbest);
    for (int j = 0; j <= 6; ++j) {
        const int off = (j & 1) ? (j + 1) / 2 : -(j / 2);                       // 0, +1, -1, +2, -2, +3, -3 ulps
        const float Dc = __uint_as_float(b0 + (unsigned)off);
        if (Dc >= 0.f && Dc == Dc && fits(Dc)) { *slot = Dc; return; }
    }
    atomicAdd(status, 1u);
}
__global__ void k_close_petd(float* petd, size_t n) {      // days that only ever showed night hours: any value works, take 0
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n && !(petd[i] == petd[i])) petd[i] = 0.f;
}

// ---- control vector of the calibration (mw_optimize.f90:679-777) ------------------------------------------------------------
// control_to_var: x[off + pos[k]] (fp64, optimiser space) -> cell vector (denormalised like k_denormalize), the full plane the
// downloads read, and -- when a regulariser is on -- the plane compute_jreg sees (normalise(denormalise(v)), mwd_cost.f90:284-291)
__global__ void k_control_set(float* cellv, float* full, float* jx, const double* x, const int* pos, const int* flat, int n, long off,
                              float lb, float ub, int denorm) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float v = (float)x[off + pos[k]];
    const float d = denorm ? v * (ub - lb) + lb : v;
    if (cellv) { cellv[k] = d; full[flat[k]] = d; }       // null: a flagged field the structure does not read (only the regulariser sees it)
    if (jx) jx[flat[k]] = denorm ? (d - lb) / (ub - lb) : v;
}
// var_to_control (grad = 0): the optimiser-space value of the field; gradient (grad = 1): cell gradient x (ub - lb) under
// denormalize_forward (DENORMALIZE_*_B, forward_db.f90:967-1057)
__global__ void k_control_get(double* x, const float* src, const int* pos, const int* flat, int n, long off, float lb, float ub,
                              int denorm, int grad, int from_full) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float v = src[from_full ? flat[k] : k];
    float r;
    if (grad) r = denorm ? (ub - lb) * v : v;
    else r = denorm ? (v - lb) / (ub - lb) : v;
    x[off + pos[k]] = (double)r;
}

// boundary series <-> dense message buffer [edge][Tq] float4
__global__ void k_halo_pack(float4* buf, const float4* x4, const int* slots, int nedge, int nx, int Tq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nedge * Tq) return;
    const int e = i / Tq, tb = i % Tq;
    buf[(size_t)e * Tq + tb] = x4[(size_t)tb * nx + slots[e]];
}
__global__ void k_halo_unpack(float4* x4, const float4* buf, const int* slots, int nedge, int nx, int Tq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nedge * Tq) return;
    const int e = i / Tq, tb = i % Tq;
    x4[(size_t)tb * nx + slots[e]] = buf[(size_t)e * Tq + tb];
}

// self-test of sx_fdiv against the IEEE division on pseudo-random operands: a = +-2^[-20,10) x [1,2), b in [blo, bhi)
__global__ void k_selftest_div(unsigned long long n, unsigned seed, float blo, float bhi, unsigned long long* out) {
    unsigned long long bad = 0, bad2 = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long h = (i + 1) * 0x9E3779B97F4A7C15ull + seed;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32; h *= 0x94D049BB133111EBull; h ^= h >> 29;
        const unsigned m1 = (unsigned)h & 0x7fffffu, m2 = (unsigned)(h >> 23) & 0x7fffffu;
        const int e1 = (int)((h >> 46) % 30) - 20;
        const float a0 = ldexpf(__uint_as_float(0x3f800000u | m1), e1);
        const float a = ((h >> 63) & 1) ? -a0 : a0;
        const float b = blo + (bhi - blo) * ((float)m2 * (1.0f / 8388608.0f));
        const float q = sx_fdiv(a, b), ref = a / b;
        if (q != ref) { ++bad; if (fabsf(q - ref) > fabsf(ref) * 2.4e-7f) ++bad2; }
    }
    if (bad) atomicAdd(out, bad);
    if (bad2) atomicAdd(out + 1, bad2);
}

// self-test of the per-wavefront straight-line paths of sx_math.h against the branchy forms they shortcut: out[0] = tanh results that
// differ (arguments a wavefront at a time: all small -> the fast path runs; every 7th wavefront mixed with large ones -> it must
// not), out[1] = x^y results that differ (positive normal bases, ordinary exponents; every 7th wavefront mixed with 0, 1, inf, < 0)
__global__ void k_selftest_paths(unsigned long long n, unsigned seed, unsigned long long* out) {
    unsigned long long bad_t = 0, bad_p = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long h = (i + 1) * 0x9E3779B97F4A7C15ull + seed;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32; h *= 0x94D049BB133111EBull; h ^= h >> 29;
        const bool mixed = ((i >> 6) % 7ull) == 6ull;                    // wave-uniform
        const unsigned m1 = (unsigned)h & 0x7fffffu, m2 = (unsigned)(h >> 23) & 0x7fffffu;
        // tanh argument: 2^[-70, -3) x [1, 2), either sign (|x| < ln2 / 4 = 0.173); mixed wavefronts: up to 2^5
        const int e1 = (int)((h >> 46) % (mixed ? 75u : 67u)) - 70;
        float x = ldexpf(__uint_as_float(0x3f800000u | m1), e1);
        if ((h >> 63) & 1) x = -x;
        if ((h >> 60) % 97ull == 0) x = 0.f;
        if (__float_as_uint(sx_tanhf(x, true)) != __float_as_uint(sx_tanhf(x, false))) ++bad_t;
        // power: base 2^[-30, 30) x [1, 2), exponent in (-6, 6)
        const int e2 = (int)((h >> 52) % 60u) - 30;
        float b = ldexpf(__uint_as_float(0x3f800000u | m2), e2);
        float y = ((float)(m1 >> 3) * (1.0f / 1048576.0f) - 0.5f) * 12.0f;
        if (mixed) { const unsigned k = (unsigned)(h >> 40) & 7u; if (k == 0) b = 0.f; else if (k == 1) b = 1.f; else if (k == 2) b = sx_inff(); else if (k == 3) b = -b; else if (k == 4) y = 0.f; else if (k == 5) b = 1e-41f; }
#if !SX_EXACT_LIBM      // (the exact-libm build raises powers through glibc's own algorithm: no such path)
        const float pf = sx_pow_from(sx_log2_d(b, true), b, y, true), pg = sx_pow_from(sx_log2_d(b, false), b, y, false);
        if (__float_as_uint(pf) != __float_as_uint(pg) && !(pf != pf && pg != pg)) ++bad_p;
#else
        (void)b; (void)y;
#endif
    }
    if (bad_t) atomicAdd(out, bad_t);
    if (bad_p) atomicAdd(out + 1, bad_p);
}

// elementwise evaluator of the math layer (smashx_selftest_eval): thread t evaluates element t (SMASHX_FN_DIV4: elements 4t .. 4t+3),
// so element i sits on lane i % 64 (blockDim and the grid stride are multiples of 64)
__global__ void k_selftest_eval(int fn, const float* x, const float* y, long long nt, float* o0, float* o1) {
    SX_LIBM_INIT();      // exact-libm build: the tables into LDS, as in the sweep kernels
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nt; t += (long long)gridDim.x * blockDim.x)
        sx_selftest_eval1(fn, x, y, t, o0, o1);
}

// whole-domain outputs: T4 chunk buffer -> planes of `plane` floats per time step, cell k at idx[k]
__global__ void k_domain_export(float* stage, const float* src4, const int* idx, int n, int npad, long plane, int tl0, int nb) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int tt = blockIdx.y;
    if (k >= n || tt >= nb) return;
    const int tl = tl0 + tt;
    stage[(size_t)tt * plane + idx[k]] = src4[((size_t)(tl >> 2) * npad + k) * 4 + (tl & 3)];
}
__global__ void k_fill(float* dst, float v, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

// qsim_d(g, t) from the per-gauge-cell tangent series
__global__ void k_gauge_rows(float* dst, const float* src, const int* gid, int ng, int nt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
    if (t < nt && g < ng) dst[(size_t)g * nt + t] = src[(size_t)gid[g] * nt + t];
}


// ---- RCCL, resolved at run time ------------------------------------------------------------------------------
// The library is not linked: a single-GPU host never loads it, and a host process that already holds an RCCL (PyTorch
// ships its own librccl.so.1) must not get a second copy -- dlopen by soname returns the copy already mapped.
struct RcclApi {
    void* h = nullptr;
    std::string err;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;        // optional (diagnostics: smashx_comm_info)
    decltype(&ncclGetVersion) GetVersion = nullptr;
    bool ok() const { return h != nullptr && err.empty(); }
};
RcclApi& rccl() {
    static RcclApi R;
    static bool tried = false;
    if (tried) return R;
    tried = true;
    const char* names[] = {getenv("SMASHX_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        if (!n || !n[0]) continue;
        R.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (R.h) break;
    }
    if (!R.h) { R.err = std::string("librccl.so.1 not found: ") + (dlerror() ? dlerror() : ""); return R; }
#define SX_SYM(f) do { R.f = (decltype(R.f))dlsym(R.h, "nccl" #f); if (!R.f) R.err = "librccl lacks nccl" #f; } while (0)
    SX_SYM(GetUniqueId); SX_SYM(CommInitRank); SX_SYM(CommDestroy); SX_SYM(Send); SX_SYM(Recv); SX_SYM(AllReduce);
    SX_SYM(GroupStart); SX_SYM(GroupEnd); SX_SYM(GetErrorString);
#undef SX_SYM
    R.CommCount = (decltype(R.CommCount))dlsym(R.h, "ncclCommCount");
    R.GetVersion = (decltype(R.GetVersion))dlsym(R.h, "ncclGetVersion");
    return R;
}
#define NCCLCHK(expr)                                                                                   \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess)                                                                          \
            return fail(SMASHX_E_HIP, std::string(#expr) + ": " + rccl().GetErrorString(r_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

struct SxComm {
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1, device = -1;
    hipStream_t stream = nullptr;    // collectives outside the sweeps (agreement check, cost sum)
    double* d_buf = nullptr;         // 64 doubles
    std::vector<smashx_plan*> plans; // plans whose exchange runs on this communicator: unhooked when it is destroyed
};
struct PeerSeg { int rank, first, count; };   // a run of boundary edges that share the peer rank

struct Launch { hipEvent_t a, b; int kind; double cellsteps; };

}  // namespace

struct smashx_plan {
    smashx_config cfg{};
    SxSchedule sch;
    int n = 0, npad = 0, nt = 0, ng = 0, st = 0;
    long n2 = 0;
    int M = 0;
    int Tc = 0, nchunks = 0;
    bool have_forcing = false, have_options = false, have_qobs = false, uploaded = false;
    bool chunk_ready = false, adj_ready = false;
    smashx_options opt{};
    std::vector<float> wgauge;       // the caller's weights; d_wgauge holds the effective ones (effective_wgauge)
    std::vector<int> gauge_flwacc_h;
    hipStream_t stream = nullptr;    // vertical kernels, uploads/downloads ("V stream")
    hipStream_t stream_r = nullptr;  // routing + cost kernels ("R stream"); overlaps the V stream chunk by chunk
    int Tp = 0;                      // pipeline sub-chunk length inside a storage chunk
    bool hi_tape = true;             // gr-b / gr-c: full tape of the interception level (false: sparse checkpoints, rebuilt in the reverse kernel)
    int chain_from = 1;              // first chained round
    // staging rows of the chained groups (sx_kernels.h "Staging rows"): tables of the transposition kernels, rows beyond the time blocks,
    // LDS of a wave-block's FIFOs; SMASHX_CHAIN_STAGE=0 keeps the plain rows (A/B)
    bool chain_stage = false; SxStageTables stg{}; int stg_blocks = 0, stg_rows_extra = 0; size_t stg_lds = 0;
    // kept tape of the chained slots (DESIGN.md 4 "Kept chain tape"): hr_imd of the chained launches of the storage chunks the reverse
    // sweep would recompute, [chunk][(time block + stage) mod Tc / 4][chained slot] float4, written in the first pass; optional, out of
    // the reserve (SMASHX_KEEP_CHAIN_TAPE=0/1).  With it and the staging rows the chained adjoint launch of a chunk is queued before the
    // chunk is recomputed (SMASHX_EARLY_ADJ_CHAIN=0/1)
    float* hrk = nullptr; bool hrk_tried = false, early_adj = true;
    size_t vlds_fwd = 0, vlds_adj = 0;   // experiments only (SMASHX_DEBUG_VLDS = n or nfwd,nadj): bytes of unused dynamic LDS per vertical workgroup, which
                                     // caps the vertical workgroups resident on a compute unit (occupancy experiments)
    std::vector<hipEvent_t> buf_free;    // per pipeline sub-chunk: the R stream has finished with this part of the chunk buffers
    std::vector<double> round_ncells;  // cells per routing round
    bool chain_used = false;         // a chained launch ran in the current sweep: check the stall flag afterwards
    bool chain = true;               // all routing rounds in one launch (progress counters), see sx_kernels.h
    // tile boundary exchange
    int n_out = 0, n_in = 0;
    int *d_out_x = nullptr, *d_in_x = nullptr;
    float *halo_out = nullptr, *halo_in = nullptr;   // caller-owned device buffers
    smashx_halo_fn halo_fn = nullptr; void* halo_user = nullptr;
    // native exchange (smashx_set_exchange): edges regrouped by peer rank, plan-owned message buffers
    SxComm* xcomm = nullptr;
    std::vector<PeerSeg> out_segs, in_segs;
    int *d_out_xp = nullptr, *d_in_xp = nullptr;     // exchange slots of the out / in edges in peer-grouped order
    float *x_out = nullptr, *x_in = nullptr;         // [edge][Tp/4] float4
    float* x_keep = nullptr; size_t x_keep_cap = 0;  // received inlet series of the storage chunks the reverse sweep recomputes: [chunk][sub-chunk][edge][Tp/4] float4
    std::vector<void*> allocs; std::vector<size_t> alloc_bytes;
    double bytes = 0;
    double hbm_free_at_plan = -1.0, hbm_total = -1.0;    // hipMemGetInfo when the storage-chunk length was chosen (smashx_plan_hbm)
    SxDeviceArrays A{};
    // extra device storage
    int* d_cell_flat = nullptr;      // k -> flat (row + col*nrow)
    int* d_sparse_idx = nullptr;     // k -> index in the sparse (nac) vectors
    float last_jobs_d = 0.f, last_jreg_d = 0.f;      // the two terms of the last smashx_forward_d's cost_d (smashx_tangent_terms)
    long n_sparse = 0;               // length of a sparse vector = the WHOLE grid's active cells along path (= n on an untiled plan)
    float* d_stage = nullptr;        // staging for full planes
    long stage_planes = 0;
    float* d_full[SX_NFIELDS] = {nullptr};   // full planes of the uploaded (denormalised) fields the structure reads, by field
    float* st0[SX_NSSLOTS] = {nullptr};      // initial (denormalised) states in cell order
    float* ckpt = nullptr;           // [nchunks][5][npad]
    float* d_prcp = nullptr; float* d_pet = nullptr;
    // control vector (smashx_control_*): position of cell k among the active cells in column-major order, device staging
    int* d_ctrl_pos = nullptr; double* d_ctrl = nullptr; size_t ctrl_cap = 0;
    // compact forcing (smashx_set_forcing_layout)
    smashx_forcing_layout flay{};
    unsigned short* d_prcp16 = nullptr; float* d_petd = nullptr; float* d_ratio = nullptr; unsigned* d_fstatus = nullptr;
    int ndays = 0; bool petd_open = false;
    std::vector<char> block_seen;    // device-block uploads: steps covered so far (the forcing counts as set once every step is)
    // cost
    int ngc = 0;
    std::vector<int> gauge_gid;
    int *d_gauge_gid = nullptr, *d_gauge_flwacc = nullptr;
    float *d_area = nullptr, *d_wgauge = nullptr, *d_qobs = nullptr, *d_qsim_b = nullptr, *d_cost_out = nullptr;
    SxGaugeSums* d_sums = nullptr; SxCostCoef* d_coef = nullptr;
    float* d_med = nullptr; int* d_med_idx = nullptr;    // median over negative-weight gauges
    int med_nslots = 0; int* d_med_slot = nullptr; float* d_medx = nullptr; int* d_medx_idx = nullptr;   // ... of several tiles
    smashx_reduce_fn med_fn = nullptr; void* med_user = nullptr; std::vector<int> med_slot_h;
    float jobs = 0.f;
    // signature criteria (smashx_set_signature_inputs, sx_signature.h): host copies of what decides the refusals of smashx_set_options
    // ([g][t]), the device tables, and whether they belong to the qobs / inputs / options the plan holds now
    struct Signature {
        bool have = false, have_mask = false, ready = false;
        std::vector<float> h_po; std::vector<int> h_mask;
        int maxev_cap = -1;
        int obs_s0 = -1, obs_lds = -1;   // the start step and buffers den_obs / n_obs on the device were formed with; -1: none
        SxSigArgs a{};
        float* d_po = nullptr; int *d_nev = nullptr, *d_ev = nullptr;
        float *d_probe_b = nullptr, *d_probe_gb = nullptr, *d_probe_gd = nullptr, *d_probe_keep = nullptr;     // smashx_jobs_of_qsim
    } sig;
    std::vector<float> h_qobs;       // [g][t], kept for the same purpose
    // optional whole-domain outputs of forward sweeps (host arrays owned by the caller)
    float* h_qsim_domain = nullptr; float* h_net_prcp_domain = nullptr; int dom_sparse = 0;
    bool dom_q_active = false;       // the running sweep stores every cell's discharge (forward sweeps only)
    // tangent sweep (smashx_forward_d)
    bool tan_ready = false;
    float* d_qsim_d = nullptr;       // [ng][nt]
    float* d_tanplane[SMASHX_GNP + SMASHX_GNS] = {nullptr};   // full planes of the (denormalised) direction, jreg only
    // regularisation (sx_jreg.h): planes 0..15 = parameters, 16..23 = states
    bool tiled = false;
    int* d_active = nullptr;
    hipStream_t stream_j = nullptr;
    hipEvent_t ev_j = nullptr;
    float* d_jx[SMASHX_GNP + SMASHX_GNS] = {nullptr};     // values as compute_cost sees them (normalised when denormalize_forward)
    float* d_jb[SMASHX_GNP + SMASHX_GNS] = {nullptr};     // background
    float* d_jg[SMASHX_GNP + SMASHX_GNS] = {nullptr};     // d(wjreg jreg)/d(field): what COMPUTE_COST_B leaves in parameters_b / states_b
    float* d_jterm = nullptr; size_t jterm_planes = 0;
    float* d_jsum = nullptr;
    SxJregChains jchains{};
    bool jr_ready = false;                                 // planes of the current upload are on the device
    // timing
    std::vector<Launch> launches;
    std::vector<hipEvent_t> pool; size_t pool_used = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    smashx_timing timing{};
    int last_adjoint = 0;
    // D8 codes of EVERY cell of the grid, active or not (0 = none): the forest of the sample paths reads them at the plan's cells,
    // mask_upstream_cells follows them all.  The host tables below are built by sx_tablehost.h on first use
    std::vector<signed char> h_flwdir_grid;
    // catchment means of the forcing (smashx_mean_forcing): the per-gauge lists of plan cells, the running sums between launches
    struct MeanForcing {
        int state = 0;                   // 0 = not built, 1 = ready, 2 = refused (a catchment leaves the active cells)
        std::string refusal;
        SxCatchments c;                  // the lists as uploaded (smashx_prcp_indices builds its own from them)
        int *d_list = nullptr, *d_begin = nullptr;
        float *d_state = nullptr, *d_mp = nullptr, *d_me = nullptr;
    } mf;
    // precipitation indices (smashx_prcp_indices): per gauge the catchment and the ten distance bins as one padded list, the catchment's
    // distances, the gauge constants; rebuilt when the caller's flwdst plane differs from the one they were built for
    struct PrcpIndices {
        int state = 0;                   // 0 = not built, 1 = ready for h_flwdst
        std::vector<float> h_flwdst;
        SxPiHost h;                      // its list, dl and d2l live on the device only
        int* d_list = nullptr; float *d_dl = nullptr, *d_d2l = nullptr; SxPiGauge* d_gauges = nullptr;
        float *d_state = nullptr, *d_out = nullptr; int* d_flag = nullptr;
    } pi;
    // what the two regional maps (smashx_hyper_*, smashx_ann_*) hold alike: the descriptors in plan-cell order, the host copy they are
    // compared with, the plan cells in the order of the adjoint's sums (set_descriptors); events and times of map and gradient (timed_*)
    struct Descriptors {
        bool have = false; int nd = 0;
        std::vector<float> h_desc;               // [nd][n], as gathered
        float* d_desc = nullptr; size_t desc_cap = 0; int* d_order = nullptr;
    };
    struct MapTiming { hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; float map_ms = 0.f, grad_ms = 0.f; };
    // hyper maps on the device (smashx_hyper_*, sx_hypermap.h): the descriptors, the hyper matrices (nh, 24), the staging rows of a span
    // and the chains
    struct Hyper {
        Descriptors dsc; MapTiming tm;
        bool mapped = false;                     // a smashx_hyper_upload has run with the descriptors held
        bool options = false;                    // smashx_set_options has been called (the plan's default options carry no bounds)
        int mapping = 0, nh = 0;
        float* d_h = nullptr; size_t h_cap = 0;
        float* d_terms = nullptr; size_t terms_cap = 0;
        float* d_sums = nullptr; size_t sums_cap = 0;
        float* d_tmp = nullptr;                  // a cell vector for the fields without a slot (smashx_hyper_fields)
        int nchain = 0, span = 0;
    } hyp;
    // the ANN regionalisation on the device (smashx_ann_*, sx_annmap.h): its own descriptors, the graph, the packed weights, cell vectors
    // for the control fields without a slot, the staging rows of a span
    struct Ann {
        Descriptors dsc; MapTiming tm;
        bool have_net = false, mapped = false;   // mapped: a smashx_ann_upload has run with the descriptors and the net held
        SxAnnNet net{};
        int field[SX_ANN_MAXCV] = {0};
        double* d_w = nullptr; size_t w_cap = 0;
        float* d_extra = nullptr; size_t extra_cap = 0;
        double* d_terms = nullptr; size_t terms_cap = 0;
        double* d_sums = nullptr; size_t sums_cap = 0;
        int span = 0;
    } ann;
    // ensemble path (smashx_multiple_run): tables built and buffers allocated on first use, all its own
    struct Ens {
        bool tables = false;
        SxForest forest;
        int *d_up = nullptr, *d_upn = nullptr, *d_order = nullptr, *d_gauge_k = nullptr;
        float *base = nullptr, *plane = nullptr;
        float *sample = nullptr, *state = nullptr, *qt = nullptr, *qg = nullptr, *gj = nullptr, *cost = nullptr, *qout = nullptr;
        size_t cap_sample = 0, cap_state = 0, cap_qt = 0, cap_qg = 0, cap_gj = 0, cap_cost = 0, cap_qout = 0;
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        int info[4] = {0, 0, 0, 0};      // batch size, time chunk, batches, chunks per batch of the last call
        float device_ms = 0.f;
        // catchment-resident path (smashx_uniform_costs, sx_resident.h): the per-thread tables built from the forest
        int res_state = 0;               // 0 = not built, 1 = ready, 2 = refused (res_refusal says why)
        std::string res_refusal;
        int *r_cell = nullptr, *r_level = nullptr, *r_upline = nullptr, *r_upn = nullptr, *r_ownline = nullptr, *r_gfirst = nullptr, *r_gnext = nullptr;
        int res_block = 0; size_t res_lds = 0, res_static = 0;
        int res_info[4] = {0, 0, 0, 0};  // cells, levels, workgroup size, LDS bytes of the last call
        float res_ms = 0.f;
    } ens;

    template <class T> int dmalloc(T** p, size_t count) {
        void* q = nullptr;
        const size_t b = std::max<size_t>(count, 1) * sizeof(T);
        hipError_t e = hipMalloc(&q, b);
        if (e != hipSuccess) return fail(SMASHX_E_HIP, std::string("hipMalloc(") + std::to_string(b) + " B): " + hipGetErrorString(e));
        allocs.push_back(q); alloc_bytes.push_back(b); bytes += (double)b; *p = (T*)q;
        return 0;
    }
    void dfree(void* q) {
        if (!q) return;
        for (size_t i = 0; i < allocs.size(); ++i)
            if (allocs[i] == q) { bytes -= (double)alloc_bytes[i]; allocs.erase(allocs.begin() + i); alloc_bytes.erase(alloc_bytes.begin() + i); break; }
        (void)hipFree(q);
    }
    template <class T> int upload_vec(T** p, const std::vector<T>& v) {
        int rc = dmalloc(p, v.size()); if (rc) return rc;
        if (!v.empty()) HIPCHK(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    hipEvent_t event() {
        if (pool_used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[pool_used++];
    }
    hipStream_t cur = nullptr;       // stream of the launch being marked
    void mark_begin(int kind, hipStream_t st, double cellsteps = 0.0) {
        cur = st; Launch l; l.a = event(); l.b = nullptr; l.kind = kind; l.cellsteps = cellsteps;
        if (l.a) (void)hipEventRecord(l.a, st);
        launches.push_back(l);
    }
    void mark_end() { Launch& l = launches.back(); l.b = event(); if (l.b) (void)hipEventRecord(l.b, cur); }
};

namespace {

int set_device(const smashx_plan* p) {
    if (p->cfg.device >= 0) HIPCHK(hipSetDevice(p->cfg.device));
    return 0;
}
// a device buffer that only grows: at least `need` elements behind *buf, *cap of them held
template <class T> int dev_grow(smashx_plan* p, T** buf, size_t* cap, size_t need) {
    if (*cap >= need) return 0;
    if (*buf) p->dfree(*buf);
    *buf = nullptr; *cap = 0;
    int rc = p->dmalloc(buf, need); if (rc) return rc;
    *cap = need;
    return 0;
}
int env_int(const char* name) { const char* e = getenv(name); return e ? std::max(0, atoi(e)) : 0; }      // a length from the environment; 0: none

// ---- fields (sx_fields.h) on this plan ------------------------------------------------------------------------------------------
// The cell vectors of a slot: its values, the values a sweep starts from (the uploaded states; a parameter's are its values) and its
// gradient, which doubles as the tangent.  References, resolved at use: the gradient vectors are allocated on the first adjoint sweep.
struct SlotVecs { float*& val; float*& start; float*& grad; };
SlotVecs slot_vecs(smashx_plan* p, int slot) {
    SxDeviceArrays& A = p->A;
    float*& val = sx_slot_vec(A, slot, false);
    return {val, sx_slot_is_state(slot) ? p->st0[slot - SX_NPSLOTS] : val, sx_slot_vec(A, slot, true)};
}
hipStream_t slot_stream(const smashx_plan* p, int slot) { return sx_slot_on_routing(slot) ? p->stream_r : p->stream; }
// what the options and the caller's structures hold for field idx (0..23)
int jreg_optim(const smashx_plan* p, int idx) {
    return idx < SMASHX_GNP ? p->opt.optim_parameters[idx] : p->opt.optim_states[idx - SMASHX_GNP];
}
float field_lb(const smashx_plan* p, int idx) { return idx < SMASHX_GNP ? p->opt.lb_parameters[idx] : p->opt.lb_states[idx - SMASHX_GNP]; }
float field_ub(const smashx_plan* p, int idx) { return idx < SMASHX_GNP ? p->opt.ub_parameters[idx] : p->opt.ub_states[idx - SMASHX_GNP]; }
float jreg_span(const smashx_plan* p, int idx) { return field_ub(p, idx) - field_lb(p, idx); }
float* host_plane(const smashx_parameters* params, const smashx_states* states, int idx) {     // null: no structure, or no plane in it
    if (idx < SMASHX_GNP) return params ? params->f[idx] : nullptr;
    return states ? states->f[idx - SMASHX_GNP] : nullptr;
}

// Levels of the river tree a routing wavefront resolves inside ONE super-step (sx_plan.h "components"): SMASHX_SUBLEVELS for the
// rounds >= 1, SMASHX_SUBLEVELS_R0 for round 0.  Default 1 = one level per super-step.  Measured (profiles/r3_sublevels.json): with 4
// levels the groups are 3.5 x shallower (335 -> 96 stages) and every result is bit-identical, but a super-step then runs its body four
// times -- 0.7 us + 0.45 us per pass, against 1.15 us for one level -- so what the fill gains the steady state loses: 1024^2 x 8760
// 157.5 -> 160.7 ms, a 2048 x 1024 tile 354 -> 375 ms; in round 0 (vector-bound) it costs 22 ms.  Kept as a switch.
int sublevels_env() {
    const char* e = getenv("SMASHX_SUBLEVELS");
    const char* e0 = getenv("SMASHX_SUBLEVELS_R0");
    return (e ? std::max(1, atoi(e)) : 1) | ((e0 ? std::max(1, atoi(e0)) : 1) << 8);
}

int chunk_len(const smashx_plan* p, int c) { return std::min(p->Tc, p->nt - c * p->Tc); }
int chain_first(const smashx_plan* p);

// allocate the time-chunk buffers; Tc from cfg or from free HBM
int ensure_chunk_buffers(smashx_plan* p, bool adjoint) {
    const int st = p->st;
    // taped levels per cell-step: hp, hft (+ hst in gr-c, + husl1 in vic-a) and, for gr-b / gr-c, the interception level hi.
    // hi depends on the forcing only: when its tape is what keeps the period from fitting in one storage chunk, the plan
    // keeps one checkpoint per SX_HIK steps instead and the reverse kernel rebuilds the levels block by block
    // (slower per step, but no recomputation of whole chunks: gr-c at 1024^2 x 8760 230 -> 204 ms).  SMASHX_HI_TAPE=0/1 forces it.
    const bool has_hi = (st == 2 || st == 3);
    const double ntape_full = (st == 5 ? 3.0 : st == 3 ? 4.0 : st == 2 ? 3.0 : 2.0);
    const double ntape_lean = has_hi ? ntape_full - 1.0 + 1.0 / SX_HIK : ntape_full;
    double ntape = ntape_full;
    if (!p->chunk_ready) {
        // a tile's neighbours must cut time exactly like it does (one message per sub-chunk): lengths sized from this
        // rank's own free HBM would differ between ranks and end in mismatched send/recv sizes
        if ((p->n_out > 0 || p->n_in > 0) && p->cfg.chunk_steps <= 0)
            return fail(SMASHX_E_ARG, "a tile with boundary series needs an explicit chunk_steps (identical on every rank; pipe_steps = 0 then means no sub-chunks)");
        const int nt16 = (p->nt + 15) / 16 * 16;
        int Tc = p->cfg.chunk_steps > 0 ? (p->cfg.chunk_steps + 15) / 16 * 16 : 0;
        {
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            p->hbm_free_at_plan = (double)fr; p->hbm_total = (double)tot;
        }
        if (Tc == 0) {
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            const double avail = (double)fr * 0.85 - 1.0e9;
            // floats per time step: qt, hr_imd and the taped levels of every cell, the exchange series (the staging rows of the chained
            // groups are optional and come out of the reserve: below)
            auto fit = [&](double nt_) { return (long)(avail / (4.0 * ((double)p->npad * (2 + nt_) + (double)std::max(p->sch.nxslots, 1)))) / 16 * 16; };
            long t = fit(ntape_full);
            if (has_hi && t < nt16) {
                // Dropping the hi tape costs the reverse kernel ~14 % (levels rebuilt block by block: 78.5 against 69 ms per 9.2e9
                // cell-steps, profiles/r3_*_2048*), one more storage chunk costs 1/C of a forward pass (~0.67 of a reverse pass): lean
                // only where it saves enough recomputation -- always when it lets the whole period fit one chunk (gr-c at 1024^2:
                // 230 -> 204 ms), not at 2048^2 where 4 lean chunks lose to 5 taped ones (784 -> see DESIGN.md 8)
                const long tl = fit(ntape_lean);
                auto nch = [&](long tc) { tc = std::max<long>(16, std::min<long>(nt16, tc)); return (double)((p->nt + tc - 1) / tc); };
                if (0.67 * (1.0 / nch(tl) - 1.0 / nch(t)) > 0.14) { p->hi_tape = false; t = tl; }
            }
            Tc = (int)std::max<long>(16, std::min<long>(nt16, t));
        }
        if (const char* e = getenv("SMASHX_HI_TAPE")) p->hi_tape = atoi(e) != 0;
        if (!has_hi) p->hi_tape = true;
        ntape = p->hi_tape ? ntape_full : ntape_lean;
        (void)ntape;
        Tc = std::min(Tc, nt16);
        {   // balance the chunks: same count, equal lengths
            const int nch = (p->nt + Tc - 1) / Tc;
            Tc = std::min(Tc, ((p->nt + nch - 1) / nch + 15) / 16 * 16);
        }
        p->Tc = Tc;
        p->A.Tc = Tc;
        p->A.hr_rows = Tc / 4;
        p->A.nx = std::max(p->sch.nxslots, 1);
        p->nchunks = (p->nt + Tc - 1) / Tc;
        {   // optional pipeline sub-chunks (V stream || R stream), equal lengths, multiples of 16.  Default: none --
            // measured at 1024^2 x 8760: overlapping the latency-bound routing groups with the vertical kernel
            // costs more (routing fill per sub-chunk, wave slots taken from the vertical kernel) than it hides.
            int want = p->cfg.pipe_steps > 0 ? p->cfg.pipe_steps : Tc;
            const int nsub = std::max(1, (Tc + want / 2) / want);
            p->Tp = std::min(Tc, ((Tc + nsub - 1) / nsub + 15) / 16 * 16);
        }
        int rc;
        if ((rc = p->dmalloc(&p->A.qtT, (size_t)p->npad * Tc))) return rc;
        if ((rc = p->dmalloc(&p->A.xT, (size_t)std::max(p->sch.nxslots, 1) * Tc))) return rc;
        HIPCHK(hipMemsetAsync(p->A.qtT, 0, (size_t)p->npad * Tc * 4, p->stream));
        HIPCHK(hipMemsetAsync(p->A.xT, 0, (size_t)std::max(p->sch.nxslots, 1) * Tc * 4, p->stream));
        p->chunk_ready = true;
    }
    if (p->h_qsim_domain && !p->A.qdT) {
        int rc;
        if ((rc = p->dmalloc(&p->A.qdT, (size_t)p->npad * p->Tc))) return rc;
    }
    if (adjoint && !p->adj_ready) {
        int rc;
        const size_t cs = (size_t)p->npad * p->Tc;
        if (p->A.qsk) { p->dfree(p->A.qsk); p->A.qsk = nullptr; }      // (taken by a forward-only sweep before: the tapes go first)
        {   // the hr_imd tape is written and read by the routing kernels only: its rows are shifted by the cell's stage and wrap at the
            // rows of the chunk, so the shift costs no memory -- never changes results (SMASHX_HR_SKEW=0: the plain rows, for A/B)
            const char* e = getenv("SMASHX_HR_SKEW");
            p->A.hr_skew = e ? atoi(e) != 0 : true;
            if ((rc = p->dmalloc(&p->A.hrT, cs))) return rc;
        }
        if ((rc = p->dmalloc(&p->A.tape_hp, cs))) return rc;
        if ((rc = p->dmalloc(&p->A.tape_hft, cs))) return rc;
        if (st == 5 || ((st == 2 || st == 3) && p->hi_tape)) { if ((rc = p->dmalloc(&p->A.tape_hi, cs))) return rc; }
        else if (st == 2 || st == 3) { if ((rc = p->dmalloc(&p->A.ckpt_hi, cs / SX_HIK))) return rc; }
        if (st == 3) { if ((rc = p->dmalloc(&p->A.tape_hst, cs))) return rc; }
        if (p->nchunks > 1) { if ((rc = p->dmalloc(&p->ckpt, (size_t)p->nchunks * SX_NSSLOTS * p->npad))) return rc; }
        for (int s = 0; s < SX_NSLOTS; ++s) if ((rc = p->dmalloc(&slot_vecs(p, s).grad, (size_t)p->npad))) return rc;
        if ((rc = p->dmalloc(&p->A.qgb, (size_t)std::max(p->ngc, 1) * p->nt))) return rc;
        if ((rc = p->dmalloc(&p->d_qsim_b, (size_t)std::max(p->ng, 1) * p->nt))) return rc;
        p->adj_ready = true;
    }
    if (p->A.ncs > 0 && !p->A.qsk) {
        // staging rows of the chained groups, [Tc / 4 + deepest chained group + 1][ncs] float4: a copy that makes the chained launches
        // faster, nothing depends on it -- it takes what the reserve holds once everything else is in place (2048^2: 7.4 GB of the
        // 34 GB the chunk length leaves free) and is left out when that is not there (the chained launches keep the plain rows)
        const size_t need = (size_t)p->A.ncs * 16 * ((size_t)p->Tc / 4 + p->stg_rows_extra + 1);
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        if ((double)fr > (double)need + 2.0e9) { int rc; if ((rc = p->dmalloc(&p->A.qsk, need / 4))) return rc; }
    }
    if (adjoint && !p->hrk_tried) {
        // kept tape of the chained slots, allocated last: what the reserve still holds after the staging rows (2048^2: 16.9 GB, less
        // than the 22.7 GB of shifted rows the routing tape no longer needs).  Untiled plans without pipeline sub-chunks only.
        p->hrk_tried = true;
        const int cf = chain_first(p);
        const char* e = getenv("SMASHX_KEEP_CHAIN_TAPE");
        const bool want = e ? atoi(e) != 0 : true;
        if (const char* ea = getenv("SMASHX_EARLY_ADJ_CHAIN")) p->early_adj = atoi(ea) != 0;
        if (want && p->nchunks > 1 && cf < p->sch.nrounds && !p->tiled && p->n_in == 0 && p->n_out == 0 && p->Tp >= p->Tc) {
            const int kcs0 = p->sch.g_slot_begin[p->sch.round_group_begin[cf]], kncs = p->sch.nslots - kcs0;
            const size_t need = (size_t)(p->nchunks - 1) * (size_t)(p->Tc / 4) * (size_t)kncs * 16;
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            if (kncs > 0 && (double)fr > (double)need + 2.0e9) {
                int rc; if ((rc = p->dmalloc(&p->hrk, need / 4))) return rc;
                p->A.kcs0 = kcs0; p->A.kncs = kncs;
            }
        }
    }
    return 0;
}

// view of the chunk buffers shifted to local step `off` (multiple of 4) of the current storage chunk
SxDeviceArrays view_at(const smashx_plan* p, int off) {
    SxDeviceArrays B = p->A;
    B.k0 = 0; B.k1 = p->n;
    const size_t q = (size_t)(off / 4);
    B.qtT = p->A.qtT + q * p->npad * 4;
    B.hrk = nullptr;                     // (the chained launches of a kept chunk set it)
    if (p->A.hrT) { if (p->A.hr_skew) B.hr_row0 = (int)q; else B.hrT = p->A.hrT + q * p->npad * 4; }
    if (p->A.qdT) B.qdT = p->A.qdT + q * p->npad * 4;
    if (!p->chain) B.qsk = nullptr;      // the launch-per-round fallback reads and writes the plain rows
    B.xT = p->A.xT + q * p->A.nx * 4;
    if (p->A.qtdT) B.qtdT = p->A.qtdT + q * p->npad * 4;      // tangent sweep (smashx_forward_d)
    if (p->A.xdT) B.xdT = p->A.xdT + q * p->A.nx * 4;
    if (p->A.tape_hp) B.tape_hp = p->A.tape_hp + (size_t)off * p->npad;
    if (p->A.tape_hft) B.tape_hft = p->A.tape_hft + (size_t)off * p->npad;
    if (p->A.tape_hi) B.tape_hi = p->A.tape_hi + (size_t)off * p->npad;
    if (p->A.ckpt_hi) B.ckpt_hi = p->A.ckpt_hi + (size_t)(off / SX_HIK) * p->npad;
    if (p->A.tape_hst) B.tape_hst = p->A.tape_hst + (size_t)off * p->npad;
    return B;
}

// ---- vertical kernels: one dispatch per family (forward, reverse, tangent), one launch for all -----------------------------------
// (structure, tape, compact forcing) -> kernel; vic-a (structure 5) is a row like the others
typedef void (*VertKernel)(SxDeviceArrays, int, int);
VertKernel vert_fwd_kernel(int st, bool tape, bool compact) {
#define SX_GR(ST) {sx_k_vert_fwd<ST, false, false>, sx_k_vert_fwd<ST, false, true>, sx_k_vert_fwd<ST, true, false>, sx_k_vert_fwd<ST, true, true>}
    static const VertKernel k[5][4] = {SX_GR(1), SX_GR(2), SX_GR(3), SX_GR(4),
                                       {sx_k_vert_fwd_vic<false, false>, sx_k_vert_fwd_vic<false, true>, sx_k_vert_fwd_vic<true, false>, sx_k_vert_fwd_vic<true, true>}};
#undef SX_GR
    return k[st - 1][2 * tape + compact];
}
VertKernel vert_adj_kernel(int st, bool compact) {
    static const VertKernel k[5][2] = {{sx_k_vert_adj<1, false>, sx_k_vert_adj<1, true>}, {sx_k_vert_adj<2, false>, sx_k_vert_adj<2, true>},
                                       {sx_k_vert_adj<3, false>, sx_k_vert_adj<3, true>}, {sx_k_vert_adj<4, false>, sx_k_vert_adj<4, true>},
                                       {sx_k_vert_adj_vic<false>, sx_k_vert_adj_vic<true>}};
    return k[st - 1][compact];
}
VertKernel vert_tan_kernel(int st) {
    static const VertKernel k[5] = {sx_k_vert_fwd_d<1>, sx_k_vert_fwd_d<2>, sx_k_vert_fwd_d<3>, sx_k_vert_fwd_d<4>, sx_k_vert_fwd_vic_d};
    return k[st - 1];
}
// one vertical launch over every cell of the plan (cells are numbered in routing-group order: round 0 first) at local step `off` of the
// storage chunk; kind: 0 forward / tangent, 3 reverse (timing)
void launch_vert(smashx_plan* p, VertKernel k, int kind, size_t lds, int off, int t0, int T) {
    const SxDeviceArrays B = view_at(p, off);
    if (B.k1 <= B.k0) return;
    const dim3 grid((B.k1 - B.k0 + SX_VBLOCK - 1) / SX_VBLOCK), block(SX_VBLOCK);
    p->mark_begin(kind, p->stream, (double)(B.k1 - B.k0) * T);
    hipLaunchKernelGGL(k, grid, block, lds, p->stream, B, t0, T);
    p->mark_end();
}
// lds: unused dynamic LDS that caps the resident vertical workgroups per compute unit (SMASHX_DEBUG_VLDS; the GR kernels only)
void vert_fwd(smashx_plan* p, int off, bool tape, int t0, int T) {
    launch_vert(p, vert_fwd_kernel(p->st, tape, p->A.prcp16 != nullptr), 0, p->st == 5 ? 0 : p->vlds_fwd, off, t0, T);
}
void vert_adj(smashx_plan* p, int off, int t0, int T) {
    launch_vert(p, vert_adj_kernel(p->st, p->A.prcp16 != nullptr), 3, p->st == 5 ? 0 : p->vlds_adj, off, t0, T);
}
void vert_tan(smashx_plan* p, int off, int t0, int T) { launch_vert(p, vert_tan_kernel(p->st), 0, 0, off, t0, T); }
double round_cells(const smashx_plan* p, int r0, int r1) {   // cells (inlets excluded) of the groups of rounds [r0, r1)
    double c = 0.0;
    for (int r = r0; r < r1; ++r) c += p->round_ncells[r];
    return c;
}
int chain_first(const smashx_plan* p) {       // first chained round (nrounds: none)
    const int nr = p->sch.nrounds;
    return (p->chain && nr - p->chain_from >= 2) ? p->chain_from : nr;
}
// counters of a chained launch: the groups' progress and the ticket counter (the stall flag lives for the whole sweep)
void reset_chain_counters(smashx_plan* p, hipStream_t st) {
    (void)hipMemsetAsync(p->A.prog, 0, (size_t)p->sch.ngroups * sizeof(int), st);
    (void)hipMemsetAsync(p->A.prog + p->sch.ngroups + 1, 0, sizeof(int), st);
}
// rounds [r0, r1) of one forward pass over [t0, t0 + T): one launch per round on stream st.  A sweep runs its un-chained rounds
// [0, chain_first) like this.  tan: 0, or the pass of the tangent sweep over every round -- 1 values in forward_d's primal forms with
// the hr_imd tape on, 2 tangents -- with every series in its plain row
void route_fwd_rounds(smashx_plan* p, int off, bool tape, int t0, int T, hipStream_t st, int r0, int r1, int tan = 0) {
    SxDeviceArrays B = view_at(p, off);
    if (!p->dom_q_active) B.qdT = nullptr;
    if (tan) B.qsk = nullptr;
    const size_t lds = (size_t)2 * p->M * sizeof(float4);
    void (*const k)(SxDeviceArrays, int, int, int, int) = tan == 1 ? sx_k_route_fwd<true, false, 1> : tan == 2 ? sx_k_route_fwd<false, false, 2>
                                                         : tape ? sx_k_route_fwd<true, false> : sx_k_route_fwd<false, false>;
    for (int r = r0; r < r1; ++r) {
        const int g0 = p->sch.round_group_begin[r], ngr = p->sch.round_group_begin[r + 1] - g0;
        p->mark_begin(1, st, round_cells(p, r, r + 1) * T);
        hipLaunchKernelGGL(k, dim3(ngr), dim3(p->M), lds, st, B, g0, g0 + ngr, t0, T);
        p->mark_end();
    }
}
// the chained rounds in ONE launch (tickets: sx_kernels.h)
// inputs_read (optional): recorded on st as soon as the pass has read the last of qtT -- after the copy into the staging rows when the
// chained launch runs on those (it then touches no buffer of the vertical kernels), else left alone (the caller records after the pass)
// hrk (optional): this chunk's part of the kept tape -- the launch tapes into it (whatever `tape` says)
bool route_fwd_chained(smashx_plan* p, int off, bool tape, int t0, int T, hipStream_t st, hipEvent_t inputs_read = nullptr, float* hrk = nullptr) {
    const int nr = p->sch.nrounds, cf = chain_first(p);
    if (cf >= nr) return false;
    SxDeviceArrays B = view_at(p, off);
    if (hrk) { B.hrk = hrk; B.hr_row0 = 0; tape = true; }
    if (!p->dom_q_active) B.qdT = nullptr;
    const size_t lds = (size_t)2 * p->M * sizeof(float4);
    const int g0 = p->sch.round_group_begin[cf], g1 = p->sch.ngroups;
    reset_chain_counters(p, st);
    const int grid = g1 - g0;
    p->mark_begin(5, st, round_cells(p, cf, nr) * T);       // (the chained launch's time includes its copy pass)
    if (B.qsk)       // the chained groups' inputs -- their cells' runoff, the series handed up to them -- into the staging rows
        hipLaunchKernelGGL((sx_k_chain_transpose<true>), dim3((p->stg_blocks + SX_STG_WAVES - 1) / SX_STG_WAVES), dim3(64 * SX_STG_WAVES), p->stg_lds * SX_STG_WAVES, st, B, p->stg, g0, (T + SX_BT - 1) / SX_BT, p->stg_blocks, (int)p->stg_lds);
    const bool early = B.qsk && inputs_read && !B.qdT;
    if (early) (void)hipEventRecord(inputs_read, st);
    if (tape) hipLaunchKernelGGL((sx_k_route_fwd<true, true>), dim3(grid), dim3(p->M), lds, st, B, g0, g1, t0, T);
    else      hipLaunchKernelGGL((sx_k_route_fwd<false, true>), dim3(grid), dim3(p->M), lds, st, B, g0, g1, t0, T);
    p->mark_end();
    p->chain_used = true;
    return early;
}
// Routing launches of one pass (sweep_once).  Rounds below chain_first keep one launch per round (they are wide and
// HBM-bound: route_fwd_rounds / route_adj_rounds); the narrow, latency-bound rounds from there on run chained inside a single launch
// (sx_kernels.h "rounds chained inside one launch"), which turns their sum into roughly the longest of them.
// the chained adjoint launch in two parts: the launch itself (hrk: this chunk's part of the kept tape, read in place of hrT) and the
// copy out of the staging rows.  On staging rows the launch touches no buffer of the vertical kernels or of round 0, so it may be queued
// long before the copy (sweep_once, "early adjoint chain")
void route_adj_chained(smashx_plan* p, int off, int t0, int T, hipStream_t st, float* hrk = nullptr, bool launch = true, bool copy = true) {
    const int nr = p->sch.nrounds, cf = chain_first(p);
    if (cf >= nr) return;
    SxDeviceArrays B = view_at(p, off);
    if (hrk) { B.hrk = hrk; B.hr_row0 = 0; }
    const size_t lds = (size_t)2 * p->M * sizeof(float4);
    const int g0 = p->sch.round_group_begin[cf], g1 = p->sch.ngroups;
    const int grid = g1 - g0;
    if (launch) {
        reset_chain_counters(p, st);
        p->mark_begin(6, st, round_cells(p, cf, nr) * T);
        hipLaunchKernelGGL((sx_k_route_adj<true>), dim3(grid), dim3(p->M), lds, st, B, g0, g1, t0, T);
        p->mark_end();
        p->chain_used = true;
    }
    if (copy && B.qsk) {
        // qt_b of the chained cells and the adjoint series that leave the chain: from the staging rows to where the vertical kernel,
        // round 0 and the exchange expect them
        p->mark_begin(7, st);
        hipLaunchKernelGGL((sx_k_chain_transpose<false>), dim3((p->stg_blocks + SX_STG_WAVES - 1) / SX_STG_WAVES), dim3(64 * SX_STG_WAVES), p->stg_lds * SX_STG_WAVES, st, B, p->stg, g0, (T + SX_BT - 1) / SX_BT, p->stg_blocks, (int)p->stg_lds);
        p->mark_end();
    }
}
void route_adj_rounds(smashx_plan* p, int off, int t0, int T, hipStream_t st) {
    const SxDeviceArrays B = view_at(p, off);
    const size_t lds = (size_t)2 * p->M * sizeof(float4);
    const int cf = chain_first(p);
    for (int r = cf - 1; r >= 0; --r) {
        const int g0 = p->sch.round_group_begin[r], ngr = p->sch.round_group_begin[r + 1] - g0;
        p->mark_begin(2, st, round_cells(p, r, r + 1) * T);
        hipLaunchKernelGGL((sx_k_route_adj<false>), dim3(ngr), dim3(p->M), lds, st, B, g0, g0 + ngr, t0, T);
        p->mark_end();
    }
}

SxCostArgs cost_args(smashx_plan* p, float jobs_b) {
    SxCostArgs C{};
    C.ng = p->ng; C.nt = p->nt; C.s0 = p->opt.optimize_start_step - 1; C.njf = p->opt.njf;
    for (int j = 0; j < SX_MAXJF; ++j) { C.jobs_fun[j] = p->opt.jobs_fun[j]; C.wjobs_fun[j] = p->opt.wjobs_fun[j]; }
    C.dt = p->cfg.dt; C.dx = p->cfg.dx;
    C.qg = p->A.qg; C.qgb = p->A.qgb; C.ngc = p->ngc;
    C.gauge_gid = p->d_gauge_gid; C.gauge_flwacc = p->d_gauge_flwacc; C.area = p->d_area; C.wgauge = p->d_wgauge;
    C.qobs = p->d_qobs; C.qsim_b = p->d_qsim_b; C.sums = p->d_sums; C.coef = p->d_coef; C.out = p->d_cost_out;
    C.med = p->d_med; C.med_idx = p->d_med_idx;
    C.nslots = p->med_nslots; C.slot = p->d_med_slot; C.medx = p->d_medx; C.medx_idx = p->d_medx_idx;
    C.jobs_b = jobs_b;
    C.sig = p->sig.a;
    return C;
}

bool is_signature(int fun) { return fun >= SMASHX_CRC && fun <= SMASHX_ERC; }
bool wants_signature(const smashx_options& o) {
    for (int j = 0; j < o.njf; ++j) if (is_signature(o.jobs_fun[j])) return true;
    return false;
}
// checked where a sweep ENTERS (smashx_sweep, smashx_forward_d, smashx_jobs_of_qsim), before anything is launched
int signature_state(smashx_plan* p) {
    if (wants_signature(p->opt) && p->ng > 0 && !p->sig.ready)
        return fail(SMASHX_E_STATE, "signature criteria: qobs or the signature inputs changed, or the options were refused, after the last accepted smashx_set_options; set the options again");
    return 0;
}

int run_cost(smashx_plan* p, int adjoint, float cost_b, float* qsim_b = nullptr, float* qgb = nullptr) {
    if (p->ng == 0 && p->med_nslots == 0) return 0;      // (a tile without gauges still takes part in the sum of the median's slots)
    SxCostArgs C = cost_args(p, cost_b);
    if (qsim_b) { C.qsim_b = qsim_b; C.qgb = qgb; }      // smashx_jobs_of_qsim: seeds into buffers of its own
    p->mark_begin(4, p->stream_r);
    if (p->ng > 0) hipLaunchKernelGGL(sx_k_cost_sums, dim3(p->ng), dim3(64), 0, p->stream_r, C);
    if (p->ng > 0 && (C.sig.want & (SX_SIG_WANT_CRC | SX_SIG_WANT_EVENTS))) hipLaunchKernelGGL(sx_k_sig_sums, dim3(p->ng), dim3(64), 0, p->stream_r, C);
    if (p->ng > 0 && (C.sig.want & SX_SIG_WANT_PCT))
        hipLaunchKernelGGL(sx_k_sig_pct, dim3(p->ng), dim3(SX_SIG_PCT_THREADS), C.sig.lds ? (size_t)(p->nt - C.s0) * 8 : 0, p->stream_r, C);
    if (p->med_nslots > 0) {
        // the median spans several tiles: local gauge_jobs into their slots, slots summed over the ranks, then the median of all
        HIPCHK(hipMemsetAsync(p->d_medx, 0, (size_t)p->med_nslots * sizeof(float), p->stream_r));
        hipLaunchKernelGGL(sx_k_cost_final, dim3(1), dim3(1), 0, p->stream_r, C, adjoint, 1);
        if (p->xcomm) {
            NCCLCHK(rccl().AllReduce(p->d_medx, p->d_medx, (size_t)p->med_nslots, ncclFloat, ncclSum, p->xcomm->comm, p->stream_r));
        } else if (p->med_fn) {
            std::vector<float> h(p->med_nslots);
            HIPCHK(hipMemcpyAsync(h.data(), p->d_medx, h.size() * sizeof(float), hipMemcpyDeviceToHost, p->stream_r));
            HIPCHK(hipStreamSynchronize(p->stream_r));
            if (p->med_fn(p->med_user, h.data(), p->med_nslots)) return fail(SMASHX_E_ARG, "median reduce callback failed");
            HIPCHK(hipMemcpyAsync(p->d_medx, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, p->stream_r));
            HIPCHK(hipStreamSynchronize(p->stream_r));
        } else return fail(SMASHX_E_STATE, "median over the gauges of several tiles: no exchange to sum the slots (smashx_set_exchange or a reduce_fn)");
        hipLaunchKernelGGL(sx_k_cost_final, dim3(1), dim3(1), 0, p->stream_r, C, adjoint, 2);
    } else
        hipLaunchKernelGGL(sx_k_cost_final, dim3(1), dim3(1), 0, p->stream_r, C, adjoint, 0);
    if (adjoint && p->ng > 0) {
        const dim3 b(256), g1((p->nt + 255) / 256, p->ng), g2((p->nt + 255) / 256, p->ngc);
        hipLaunchKernelGGL(sx_k_cost_seeds, g1, b, 0, p->stream_r, C);
        hipLaunchKernelGGL(sx_k_cost_cellseeds, g2, b, 0, p->stream_r, C);
    }
    p->mark_end();
    return 0;
}

// The states of the structure between their cell vectors and a kept copy: the uploaded states (c < 0) or the checkpoint taken before
// storage chunk c.  The reservoir levels move on the V stream, the routing store hlr on the R stream (sx_fields.h).
int move_states(smashx_plan* p, int c, bool save) {
    for (int s = SX_NPSLOTS; s < SX_NSLOTS; ++s) {
        if (sx_slot_field(p->st, s) < 0) continue;
        const SlotVecs V = slot_vecs(p, s);
        float* const kept = c < 0 ? V.start : p->ckpt + ((size_t)c * SX_NSSLOTS + (s - SX_NPSLOTS)) * p->npad;
        HIPCHK(hipMemcpyAsync(save ? kept : V.val, save ? V.val : kept, (size_t)p->npad * 4, hipMemcpyDeviceToDevice, slot_stream(p, s)));
    }
    return 0;
}
int restore_states(smashx_plan* p, int c = -1) { return move_states(p, c, false); }
int checkpoint_states(smashx_plan* p, int c) { return move_states(p, c, true); }

}  // namespace

extern "C" {

const char* smashx_last_error(void) { return g_err.c_str(); }

int smashx_abi_sizes(int sizes[7]) {
    if (sizes) {
        sizes[0] = (int)sizeof(smashx_config); sizes[1] = (int)sizeof(smashx_mesh); sizes[2] = (int)sizeof(smashx_options);
        sizes[3] = (int)sizeof(smashx_parameters); sizes[4] = (int)sizeof(smashx_states); sizes[5] = (int)sizeof(smashx_costs);
        sizes[6] = (int)sizeof(smashx_timing);
    }
    return SMASHX_ABI_VERSION;
}

int smashx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int smashx_plan_create(const smashx_config* cfg, const smashx_mesh* mesh, smashx_plan** out) {
    if (!cfg || !mesh || !out) return fail(SMASHX_E_ARG, "null argument");
    *out = nullptr;
    if (cfg->structure < 1 || cfg->structure > 5) return fail(SMASHX_E_UNSUPPORTED, "structure must be gr-a/b/c/d or vic-a");
    if (cfg->nrow <= 0 || cfg->ncol <= 0 || cfg->nt <= 0 || cfg->ng < 0 || !(cfg->dt > 0.f) || !(cfg->dx > 0.f))
        return fail(SMASHX_E_ARG, "bad sizes in smashx_config");
    if (!mesh->flwdir || !mesh->flwacc || !mesh->active_cell || (cfg->ng > 0 && (!mesh->gauge_pos || !mesh->area)))
        return fail(SMASHX_E_ARG, "null mesh array");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SMASHX_E_NODEVICE, "no HIP device: libsmashx has no CPU fallback");
    smashx_plan* p = new smashx_plan();
    p->cfg = *cfg;
    if (set_device(p)) { delete p; return SMASHX_E_HIP; }
    p->M = cfg->group_size > 0 ? cfg->group_size : 512;
    if (p->M % 64 != 0 || p->M > SX_MAXGROUP || p->M < 64) { delete p; return fail(SMASHX_E_ARG, "group_size must be a multiple of 64 in [64, 512]"); }
    const bool rect_tile = cfg->tile[1] > cfg->tile[0] && cfg->tile[3] > cfg->tile[2];
    const bool tiled = rect_tile || mesh->owner_mask;
    const int rc0 = sx_build_schedule(cfg->nrow, cfg->ncol, mesh->flwdir, mesh->active_cell, cfg->ng, mesh->gauge_pos, p->M,
                                      rect_tile ? cfg->tile : nullptr, p->sch, mesh->owner_mask, sublevels_env());
    if (rc0 != 0) { std::string e = p->sch.error; delete p; return fail(rc0 == -5 ? SMASHX_E_MESH : SMASHX_E_ARG, e); }
    p->tiled = tiled;
    if (!tiled) {
        p->h_flwdir_grid.resize((size_t)cfg->nrow * cfg->ncol);
        for (size_t c = 0; c < p->h_flwdir_grid.size(); ++c) { const int d = mesh->flwdir[c]; p->h_flwdir_grid[c] = (d >= 1 && d <= 8) ? (signed char)d : 0; }
    }
    p->n = p->sch.n; p->npad = (p->n + SX_VBLOCK - 1) / SX_VBLOCK * SX_VBLOCK;
    p->nt = cfg->nt; p->ng = cfg->ng; p->st = cfg->structure; p->n2 = (long)cfg->nrow * cfg->ncol;
    int rc = 0;
#define TRY(x) do { rc = (x); if (rc) { smashx_plan_destroy(p); return rc; } } while (0)
    if (hipStreamCreate(&p->stream) != hipSuccess || hipStreamCreate(&p->stream_r) != hipSuccess) { delete p; return fail(SMASHX_E_HIP, "hipStreamCreate failed"); }
    (void)hipEventCreate(&p->ev0); (void)hipEventCreate(&p->ev1);
    if (hipStreamCreate(&p->stream_j) != hipSuccess || hipEventCreate(&p->ev_j) != hipSuccess) { smashx_plan_destroy(p); return fail(SMASHX_E_HIP, "hipStreamCreate failed"); }
    SxDeviceArrays& A = p->A;
    A.n = p->n; A.npad = p->npad; A.nt = p->nt; A.dt = cfg->dt; A.dx = cfg->dx; A.Tc = 0;
    if (getenv("SMASHX_VERBOSE"))
        for (int r = 0; r < p->sch.nrounds; ++r) {       // diagnostics: shape of the routing schedule
            long slots = 0, inlets = 0, dsum = 0; int dmx = 0;
            const int ga = p->sch.round_group_begin[r], gb = p->sch.round_group_begin[r + 1];
            for (int g = ga; g < gb; ++g) {
                dsum += p->sch.g_dmax[g]; dmx = std::max(dmx, p->sch.g_dmax[g]);
                for (int q = p->sch.g_slot_begin[g]; q < p->sch.g_slot_begin[g + 1]; ++q) { if (p->sch.s_cell[q] == INT_MIN) continue; ++slots; if (p->sch.s_cell[q] < 0) ++inlets; }
            }
            fprintf(stderr, "smashx: routing round %d: %d groups, %ld slots (%ld inlets), depth mean %.1f max %d\n", r, gb - ga, slots, inlets,
                    gb > ga ? (double)dsum / (gb - ga) : 0.0, dmx);
        }
    // schedule tables
    int *d1, *d2, *d3, *d4, *d5, *d6, *d7, *d8;
    TRY(p->upload_vec(&d1, p->sch.g_slot_begin)); A.g_slot_begin = d1;
    TRY(p->upload_vec(&d2, p->sch.g_dmax)); A.g_dmax = d2;
    TRY(p->upload_vec(&d3, p->sch.s_cell)); A.s_cell = d3;
    TRY(p->upload_vec(&d4, p->sch.s_stage)); A.s_stage = d4;
    TRY(p->upload_vec(&d5, p->sch.s_child)); A.s_child = d5;
    TRY(p->upload_vec(&d6, p->sch.s_ccount)); A.s_ccount = d6;
    { int *e1, *e2; TRY(p->upload_vec(&e1, p->sch.s_sub)); A.s_sub = e1; TRY(p->upload_vec(&e2, p->sch.s_wsub)); A.s_wsub = e2; }
    TRY(p->upload_vec(&d7, p->sch.s_parent)); A.s_parent = d7;
    TRY(p->upload_vec(&d8, p->sch.s_xout)); A.s_xout = d8;
    {   // chained rounds (the rounds from SMASHX_CHAIN_FROM, default 1, share one launch); SMASHX_CHAIN_ROUNDS=0
        // restores the launch-per-round schedule for A/B measurements and bisection
        int *d9, *d10;
        TRY(p->upload_vec(&d9, p->sch.x_prod_group)); A.x_prod = d9;
        TRY(p->upload_vec(&d10, p->sch.x_cons_group)); A.x_cons = d10;
        TRY(p->dmalloc(&A.prog, (size_t)p->sch.ngroups + SX_PROG_EXTRA));
        if (hipMemset(A.prog, 0, ((size_t)p->sch.ngroups + SX_PROG_EXTRA) * sizeof(int)) != hipSuccess) { smashx_plan_destroy(p); return fail(SMASHX_E_HIP, "hipMemset"); }
        A.ngroups = p->sch.ngroups;
        const char* e = getenv("SMASHX_CHAIN_ROUNDS");
        p->chain = !(e && e[0] == '0');
        if (const char* dv = getenv("SMASHX_DEBUG_VLDS")) {       // "n" or "nfwd,nadj"
            p->vlds_fwd = p->vlds_adj = (size_t)std::max(0, atoi(dv));
            if (const char* c2 = strchr(dv, ',')) p->vlds_adj = (size_t)std::max(0, atoi(c2 + 1));
        }
        p->round_ncells.assign(p->sch.nrounds, 0.0);
        for (int r = 0; r < p->sch.nrounds; ++r)
            for (int g = p->sch.round_group_begin[r]; g < p->sch.round_group_begin[r + 1]; ++g)
                for (int q = p->sch.g_slot_begin[g]; q < p->sch.g_slot_begin[g + 1]; ++q) p->round_ncells[r] += p->sch.s_cell[q] >= 0;
        const char* cfm = getenv("SMASHX_CHAIN_FROM");
        p->chain_from = cfm ? std::max(0, atoi(cfm)) : 1;
        {   // staging rows of the chained groups: wave-blocks of 64 consecutive slots of one group, FIFO offsets per slot and direction
            A.qsk = nullptr; A.cs0 = 0; A.ncs = 0;
            const int cf = chain_first(p);
            {   // The copy pays where the chained launch is bound by its memory instructions: several waves of groups per compute unit
                // (2048^2: 1293 groups, sweep -12 ms).  A launch the device holds at once is bound by the latency of its chain of stages
                // instead, gains less than the two passes cost (1024^2: 316 groups, chained launches -5 ms, passes +6.5 ms) and keeps the
                // plain rows.  SMASHX_CHAIN_STAGE=0/1 overrides.
                int dev = 0, cus = 256;
                if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
                const int nchained = cf < p->sch.nrounds ? p->sch.ngroups - p->sch.round_group_begin[cf] : 0;
                p->chain_stage = nchained >= 2 * cus;
                if (const char* cs = getenv("SMASHX_CHAIN_STAGE")) p->chain_stage = atoi(cs) != 0;
            }
            if (p->chain_stage && cf < p->sch.nrounds) {
                const int gc = p->sch.round_group_begin[cf];
                const int cs0 = p->sch.g_slot_begin[gc], ncs = p->sch.nslots - cs0;
                std::vector<int> slot0, cnt, smn, spr, fg((size_t)std::max(ncs, 1), 0), fs((size_t)std::max(ncs, 1), 0);
                size_t lds = 0;
                int extra = 0;
                for (int g = gc; g < p->sch.ngroups; ++g) {
                    extra = std::max(extra, p->sch.g_dmax[g]);
                    const int sb = p->sch.g_slot_begin[g], m = p->sch.g_slot_begin[g + 1] - sb;
                    for (int o = 0; o < m; o += 64) {
                        const int nl = std::min(64, m - o);
                        int lo = INT_MAX, hi = 0;
                        for (int q = sb + o; q < sb + o + nl; ++q) { lo = std::min(lo, p->sch.s_stage[q]); hi = std::max(hi, p->sch.s_stage[q]); }
                        size_t og = 0, os = 0;
                        for (int q = sb + o; q < sb + o + nl; ++q) {
                            const int d = p->sch.s_stage[q] - lo;
                            fg[q - cs0] = (int)og; og += (size_t)d + 1;
                            fs[q - cs0] = (int)os; os += (size_t)(hi - lo - d) + 1;
                        }
                        lds = std::max(lds, std::max(og, os) * sizeof(float4));
                        slot0.push_back(sb + o); cnt.push_back(nl); smn.push_back(lo); spr.push_back(hi - lo);
                    }
                }
                if (lds * SX_STG_WAVES <= 160 * 1024 && lds <= 64 * 1024 && !slot0.empty()) {      // (a schedule whose wave-blocks span more stages than that keeps the plain rows)
                    int *d0, *d1, *d2, *d3, *d4, *d5;
                    TRY(p->upload_vec(&d0, slot0)); TRY(p->upload_vec(&d1, cnt)); TRY(p->upload_vec(&d2, smn)); TRY(p->upload_vec(&d3, spr));
                    TRY(p->upload_vec(&d4, fg)); TRY(p->upload_vec(&d5, fs));
                    p->stg = SxStageTables{d0, d1, d2, d3, d4, d5};
                    p->stg_blocks = (int)slot0.size(); p->stg_rows_extra = extra; p->stg_lds = (lds + 15) / 16 * 16;
                    // the copy kernels may use all of a CU's LDS (160 KiB; the attribute belongs to the kernel, not to the plan: the same
                    // value for every plan of the process).  Where that is refused, a plan that needs more than the default keeps the plain rows
                    static const bool lds_ok = []() {
                        return hipFuncSetAttribute(reinterpret_cast<const void*>(&sx_k_chain_transpose<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess
                            && hipFuncSetAttribute(reinterpret_cast<const void*>(&sx_k_chain_transpose<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
                    }();
                    if (lds_ok || p->stg_lds * SX_STG_WAVES <= 48 * 1024) { A.cs0 = cs0; A.ncs = ncs; }
                    else (void)hipGetLastError();
                }
            }
        }
        A.spin_limit = SX_SPIN_LIMIT; A.mute_group = -1;
        if (const char* sl = getenv("SMASHX_SPIN_LIMIT")) A.spin_limit = std::max(1, atoi(sl));
        if (const char* mg = getenv("SMASHX_DEBUG_MUTE_GROUP")) A.mute_group = atoi(mg);     // tests of the stall path only
        if (A.mute_group < -1) A.mute_group = p->sch.round_group_begin[std::min(p->chain_from, p->sch.nrounds - 1)];   // "the first chained group"
        A.gtime = nullptr;
        const char* tr = getenv("SMASHX_TRACE_GROUPS");
        if (tr && tr[0] == '1') {
            TRY(p->dmalloc(&A.gtime, (size_t)4 * p->sch.ngroups));
            if (hipMemset(A.gtime, 0, (size_t)4 * p->sch.ngroups * sizeof(long long)) != hipSuccess) { smashx_plan_destroy(p); return fail(SMASHX_E_HIP, "hipMemset"); }
        }
    }
    TRY(p->upload_vec(&p->d_cell_flat, p->sch.cell_flat));
    TRY(p->upload_vec(&p->d_active, std::vector<int>(mesh->active_cell, mesh->active_cell + p->n2)));
    TRY(p->dmalloc(&p->d_jsum, (size_t)SX_JREG_MAXCHAIN));
    p->n_out = (int)p->sch.out_x.size(); p->n_in = (int)p->sch.in_x.size();
    TRY(p->upload_vec(&p->d_out_x, p->sch.out_x.empty() ? std::vector<int>(1, 0) : p->sch.out_x));
    TRY(p->upload_vec(&p->d_in_x, p->sch.in_x.empty() ? std::vector<int>(1, 0) : p->sch.in_x));
    // per-cell mesh data
    std::vector<int> facc(p->npad, 1), cg(p->npad, -1);
    for (int k = 0; k < p->n; ++k) facc[k] = mesh->flwacc[p->sch.cell_flat[k]];
    p->gauge_gid.assign(p->ng, -1);
    std::vector<int> gfl(std::max(p->ng, 1), 1);
    for (int g = 0; g < p->ng; ++g) {
        const int k = p->sch.gauge_k[g];
        if (cg[k] < 0) cg[k] = p->ngc++;
        p->gauge_gid[g] = cg[k];
        gfl[g] = mesh->flwacc[p->sch.cell_flat[k]];
    }
    TRY(p->upload_vec(&A.flwacc, facc));
    TRY(p->upload_vec(&A.cell_gauge, cg));
    // sparse forcing index: k -> position along path over active cells (mw_sparse_storage.f90:12-49)
    if (mesh->path) {
        std::vector<int> sp(p->n, -1);
        int ind = 0;
        for (long i = 0; i < p->n2; ++i) {
            const int row = mesh->path[2 * i], col = mesh->path[2 * i + 1];
            if (row < 0 || col < 0 || row >= cfg->nrow || col >= cfg->ncol) continue;
            const long c = row + (long)col * cfg->nrow;
            if (mesh->active_cell[c] == 1) { const int k = p->sch.k_of_flat[c]; if (k >= 0 && sp[k] < 0) sp[k] = ind; ++ind; }
        }
        bool ok = true;
        for (int k = 0; k < p->n; ++k) ok &= sp[k] >= 0;
        if (ok) { TRY(p->upload_vec(&p->d_sparse_idx, sp)); p->n_sparse = ind; }
    }
    // parameters, states, routing invariants
    for (int s = 0; s < SX_NSLOTS; ++s) TRY(p->dmalloc(&slot_vecs(p, s).val, (size_t)p->npad));
    for (int i = 0; i < SX_NSSLOTS; ++i) TRY(p->dmalloc(&p->st0[i], (size_t)p->npad));
    float** rf[4] = {&A.rt_a, &A.rt_f, &A.rt_denf, &A.rt_denb};
    for (auto q : rf) TRY(p->dmalloc(q, (size_t)p->npad));
    for (int s = 0; s < SX_NSLOTS; ++s) if (sx_slot_field(p->st, s) >= 0) TRY(p->dmalloc(&p->d_full[sx_slot_field(p->st, s)], (size_t)p->n2));
    p->stage_planes = std::max<long>(1, std::min<long>(64, (256L << 20) / (p->n2 * 4)));
    TRY(p->dmalloc(&p->d_stage, (size_t)p->n2 * p->stage_planes));
    // gauges / cost
    TRY(p->dmalloc(&A.qg, (size_t)std::max(p->ngc, 1) * p->nt));
    TRY(p->upload_vec(&p->d_gauge_gid, p->gauge_gid.empty() ? std::vector<int>(1, 0) : p->gauge_gid));
    TRY(p->upload_vec(&p->d_gauge_flwacc, gfl));
    p->gauge_flwacc_h = gfl;
    std::vector<float> area(std::max(p->ng, 1), 1.f);
    for (int g = 0; g < p->ng; ++g) area[g] = mesh->area[g];
    TRY(p->upload_vec(&p->d_area, area));
    TRY(p->dmalloc(&p->d_wgauge, (size_t)std::max(p->ng, 1)));
    TRY(p->dmalloc(&p->d_qobs, (size_t)std::max(p->ng, 1) * p->nt));
    TRY(p->dmalloc(&p->d_sums, (size_t)std::max(p->ng, 1)));
    TRY(p->dmalloc(&p->d_coef, (size_t)std::max(p->ng, 1) * SX_MAXJF));
    TRY(p->dmalloc(&p->d_med, (size_t)2 * std::max(p->ng, 1)));
    TRY(p->dmalloc(&p->d_med_idx, (size_t)2 * std::max(p->ng, 1)));
    TRY(p->dmalloc(&p->d_cost_out, 4));
    if (hipMemset(p->d_qobs, 0, (size_t)std::max(p->ng, 1) * p->nt * 4) != hipSuccess) { smashx_plan_destroy(p); return fail(SMASHX_E_HIP, "hipMemset"); }
    // default options: plain Model.run(): njf = 0 (mwd_setup.f90:236)
    std::memset(&p->opt, 0, sizeof(p->opt));
    p->opt.optimize_start_step = 1;
    p->wgauge.assign(std::max(p->ng, 1), p->ng > 0 ? 1.f / p->ng : 0.f);
    if (hipMemcpy(p->d_wgauge, p->wgauge.data(), p->wgauge.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { smashx_plan_destroy(p); return fail(SMASHX_E_HIP, "hipMemcpy"); }
    p->have_options = true;
#undef TRY
    *out = p;
    return 0;
}

int smashx_plan_destroy(smashx_plan* p) {
    if (!p) return 0;
    (void)set_device(p);
    if (p->xcomm) { auto& v = p->xcomm->plans; v.erase(std::remove(v.begin(), v.end(), p), v.end()); }
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->stream_r) (void)hipStreamSynchronize(p->stream_r);
    for (void* q : p->allocs) (void)hipFree(q);
    for (hipEvent_t e : p->pool) (void)hipEventDestroy(e);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    if (p->stream_r) (void)hipStreamDestroy(p->stream_r);
    if (p->stream_j) { (void)hipStreamSynchronize(p->stream_j); (void)hipStreamDestroy(p->stream_j); }
    if (p->ev_j) (void)hipEventDestroy(p->ev_j);
    if (p->ens.ev_a) (void)hipEventDestroy(p->ens.ev_a);
    if (p->ens.ev_b) (void)hipEventDestroy(p->ens.ev_b);
    for (const smashx_plan::MapTiming* t : {&p->hyp.tm, &p->ann.tm})
        for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    delete p;
    return 0;
}

int smashx_plan_ncells(const smashx_plan* p) { return p ? p->n : SMASHX_E_ARG; }

int smashx_plan_cell_order(const smashx_plan* p, int* rows, int* cols) {
    if (!p || !rows || !cols) return fail(SMASHX_E_ARG, "null argument");
    for (int k = 0; k < p->n; ++k) { rows[k] = p->sch.cell_flat[k] % p->cfg.nrow; cols[k] = p->sch.cell_flat[k] / p->cfg.nrow; }
    return 0;
}

static int alloc_forcing(smashx_plan* p) {
    if (p->d_prcp || p->d_prcp16) return 0;
    int rc;
    p->block_seen.clear();           // new rows: nothing is covered yet
    if (p->flay.compact) {
        p->ndays = (p->nt + p->flay.pet_hour0 + 23) / 24;
        if ((rc = p->dmalloc(&p->d_prcp16, (size_t)p->nt * p->npad))) return rc;
        if ((rc = p->dmalloc(&p->d_petd, (size_t)p->ndays * p->npad))) return rc;
        if ((rc = p->dmalloc(&p->d_ratio, 24))) return rc;
        if ((rc = p->dmalloc(&p->d_fstatus, 2))) return rc;
        HIPCHK(hipMemset(p->d_prcp16, 0, (size_t)p->nt * p->npad * sizeof(unsigned short)));
        HIPCHK(hipMemset(p->d_petd, 0xFF, (size_t)p->ndays * p->npad * sizeof(float)));      // NaN = "day not determined yet"
        HIPCHK(hipMemset(p->d_fstatus, 0, 2 * sizeof(unsigned)));
        HIPCHK(hipMemcpy(p->d_ratio, p->flay.pet_ratio, 24 * sizeof(float), hipMemcpyHostToDevice));
        p->A.prcp16 = p->d_prcp16; p->A.petd = p->d_petd; p->A.pet_ratio = p->d_ratio;
        p->A.prcp_c = p->flay.prcp_factor; p->A.prcp_gap = -99.f; p->A.hour0 = p->flay.pet_hour0;
        p->A.prcp = nullptr; p->A.pet = nullptr;
        return 0;
    }
    if ((rc = p->dmalloc(&p->d_prcp, (size_t)p->nt * p->npad))) return rc;
    if ((rc = p->dmalloc(&p->d_pet, (size_t)p->nt * p->npad))) return rc;
    p->A.prcp = p->d_prcp; p->A.pet = p->d_pet;
    p->A.prcp16 = nullptr; p->A.petd = nullptr; p->A.pet_ratio = nullptr;
    return 0;
}

static void drop_compact(smashx_plan* p) {
    p->dfree(p->d_prcp16); p->dfree(p->d_petd); p->dfree(p->d_ratio); p->dfree(p->d_fstatus);
    p->d_prcp16 = nullptr; p->d_petd = nullptr; p->d_ratio = nullptr; p->d_fstatus = nullptr;
    p->A.prcp16 = nullptr; p->A.petd = nullptr; p->A.pet_ratio = nullptr;
    p->flay.compact = 0;
}

// encode + verify rows [t0, t0 + rows) from fp32 device rows (row stride ld, cell k at idx[k] or k); *ok = every value is
// reproduced bit for bit by the kernels' decode
static int encode_block(smashx_plan* p, int t0, int rows, const float* d_prcp_src, const float* d_pet_src, const int* idx, long ld,
                        hipStream_t st, bool* ok) {
    const int h0 = p->flay.pet_hour0;
    const int d0 = (t0 + h0) / 24, d1 = (t0 + rows - 1 + h0) / 24;
    for (int r0 = 0; r0 < rows; r0 += 32768) {      // grid.y limit
        const int rr = std::min(32768, rows - r0);
        hipLaunchKernelGGL(k_encode_prcp, dim3((p->n + 255) / 256, rr), dim3(256), 0, st, p->d_prcp16 + (size_t)(t0 + r0) * p->npad,
                           d_prcp_src + (size_t)r0 * ld, idx, p->n, p->npad, ld, rr, p->flay.prcp_factor, p->d_fstatus);
    }
    hipLaunchKernelGGL(k_encode_pet, dim3((p->n + 255) / 256, d1 - d0 + 1), dim3(256), 0, st, p->d_petd, d_pet_src, idx, p->n, p->npad, ld,
                       t0, rows, h0, p->d_ratio, p->d_fstatus);
    unsigned status[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(status, p->d_fstatus, sizeof(status), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    *ok = status[0] == 0;
    if (status[1]) { float g; std::memcpy(&g, &status[1], 4); p->A.prcp_gap = g; }
    p->petd_open = true;
    return 0;
}

int smashx_set_forcing_layout(smashx_plan* p, const smashx_forcing_layout* lay) {
    if (!p || !lay) return fail(SMASHX_E_ARG, "null argument");
    if (p->d_prcp || p->d_prcp16) {
        if (p->have_forcing && !p->d_prcp16 == !lay->compact) return fail(SMASHX_E_STATE, "the forcing is already resident in this layout");
        int rc = set_device(p); if (rc) return rc;                     // reset: drop what is resident, the caller sends the forcing again
        HIPCHK(hipStreamSynchronize(p->stream)); HIPCHK(hipStreamSynchronize(p->stream_r));
        drop_compact(p);
        p->dfree(p->d_prcp); p->dfree(p->d_pet); p->d_prcp = p->d_pet = nullptr; p->A.prcp = p->A.pet = nullptr;
        p->have_forcing = false;
        p->block_seen.clear();
    }
    if (lay->compact) {
        if (p->cfg.dt != 3600.f) return fail(SMASHX_E_UNSUPPORTED, "compact forcing: the daily-PET form is defined for dt = 3600 s");
        // (positive / non-negative AND finite: the vertical kernels tell "no lane is in a gap" from the stored words, SxForcing::no_gap)
        if (!(lay->prcp_factor > 0.f) || __builtin_isinf(lay->prcp_factor) || lay->pet_hour0 < 0 || lay->pet_hour0 > 23) return fail(SMASHX_E_ARG, "bad prcp_factor / pet_hour0");
        for (int h = 0; h < 24; ++h) if (!(lay->pet_ratio[h] >= 0.f) || __builtin_isinf(lay->pet_ratio[h])) return fail(SMASHX_E_ARG, "pet_ratio must be >= 0 and finite");
    }
    p->flay = *lay;
    return 0;
}

int smashx_forcing_info(const smashx_plan* p, int* compact, double* bytes_per_cellstep) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    const bool c = p->d_prcp16 != nullptr || (!p->d_prcp && p->flay.compact);
    if (compact) *compact = c ? 1 : 0;
    if (bytes_per_cellstep) *bytes_per_cellstep = c ? 2.0 + 4.0 * ((p->nt + p->flay.pet_hour0 + 23) / 24) / (double)p->nt : 8.0;
    return 0;
}

int smashx_set_forcing(smashx_plan* p, const float* prcp, const float* pet, int sparse) {
    if (!p || !prcp || !pet) return fail(SMASHX_E_ARG, "null argument");
    int rc = set_device(p); if (rc) return rc;
    if (sparse && !p->d_sparse_idx) return fail(SMASHX_E_ARG, "sparse forcing needs mesh.path at plan creation");
    // a sparse vector is numbered over the whole grid's active cells: on a tiled plan it is longer than the part (the part's cells
    // keep their whole-grid positions in it)
    const long plane = sparse ? p->n_sparse : p->n2;
    const int* idx = sparse ? p->d_sparse_idx : p->d_cell_flat;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = alloc_forcing(p))) return rc;
        const bool compact = p->d_prcp16 != nullptr;
        bool ok = true;
        if (compact) {
            // staged in blocks of whole days, so that a day's PET is determined from all of its hours at once; both variables of a
            // block share the staging buffer
            const long half = std::max<long>(1, p->stage_planes / 2);
            HIPCHK(hipMemsetAsync(p->d_fstatus, 0, 2 * sizeof(unsigned), p->stream));      // a fresh data set: no gap value known yet
            HIPCHK(hipMemsetAsync(p->d_petd, 0xFF, (size_t)p->ndays * p->npad * sizeof(float), p->stream));
            for (int t = 0; t < p->nt && ok;) {
                int rows = (int)std::min<long>(half, p->nt - t);
                const int to_day_end = 24 - (t + p->flay.pet_hour0) % 24;
                if (rows > to_day_end) rows = to_day_end + (rows - to_day_end) / 24 * 24;
                float* sp = p->d_stage; float* se = p->d_stage + (size_t)half * p->n2;
                HIPCHK(hipMemcpyAsync(sp, prcp + (size_t)t * plane, (size_t)rows * plane * 4, hipMemcpyHostToDevice, p->stream));
                HIPCHK(hipMemcpyAsync(se, pet + (size_t)t * plane, (size_t)rows * plane * 4, hipMemcpyHostToDevice, p->stream));
                if ((rc = encode_block(p, t, rows, sp, se, idx, plane, p->stream, &ok))) return rc;
                t += rows;
            }
            if (ok) break;
            // not of the reader's form: never approximate -- keep the fp32 rows
            HIPCHK(hipStreamSynchronize(p->stream));
            drop_compact(p);
            continue;
        }
        const float* src[2] = {prcp, pet};
        float* dst[2] = {p->d_prcp, p->d_pet};
        for (int v = 0; v < 2; ++v)
            for (int t = 0; t < p->nt; t += (int)p->stage_planes) {
                const int rows = (int)std::min<long>(p->stage_planes, p->nt - t);
                HIPCHK(hipMemcpyAsync(p->d_stage, src[v] + (size_t)t * plane, (size_t)rows * plane * 4, hipMemcpyHostToDevice, p->stream));
                hipLaunchKernelGGL(k_gather_rows, dim3((p->n + 255) / 256, rows), dim3(256), 0, p->stream,
                                   dst[v] + (size_t)t * p->npad, p->d_stage, idx, p->n, p->npad, plane, rows);
                HIPCHK(hipStreamSynchronize(p->stream));
            }
        break;
    }
    p->have_forcing = true;
    if (getenv("SMASHX_VERBOSE"))
        fprintf(stderr, "smashx: forcing resident as %s (%.2f GB for %d cells x %d steps)\n", p->d_prcp16 ? "compact uint16 rain counts + daily PET" : "fp32 rows",
                (p->d_prcp16 ? 2.0 * p->nt + 4.0 * p->ndays : 8.0 * p->nt) * p->npad * 1e-9, p->n, p->nt);
    return 0;
}

// The forcing only counts as set once device blocks have covered every step of [0, nt): a sweep started earlier would close the
// daily PET of days it has not seen (k_close_petd pins them to 0) and later blocks for those days would then fail verification.
// Coverage is only forgotten where the data it stands for is: when the rows are (re)allocated (alloc_forcing, a new layout) and -- compact
// layout only -- when a block starting at step 0 opens a new upload cycle (its daily PET field is reset there, see below).  fp32 rows may
// be sent in any order and refreshed block by block.
static void mark_block(smashx_plan* p, int t0, int t1, bool new_cycle) {
    if (new_cycle) p->block_seen.assign(p->nt, 0);
    p->block_seen.resize(p->nt, 0);
    std::fill(p->block_seen.begin() + t0, p->block_seen.begin() + t1, 1);
    p->have_forcing = std::find(p->block_seen.begin(), p->block_seen.end(), 0) == p->block_seen.end();
}

int smashx_set_forcing_device_block(smashx_plan* p, int t0, int t1, const float* d_prcp, const float* d_pet) {
    if (!p || !d_prcp || !d_pet || t0 < 0 || t1 > p->nt || t0 >= t1) return fail(SMASHX_E_ARG, "bad block");
    int rc = set_device(p); if (rc) return rc;
    if ((rc = alloc_forcing(p))) return rc;
    if (p->d_prcp16) {
        bool ok = true;
        if (t0 == 0) {   // the forcing is being sent again from its start: forget the previous data set's gap value and daily field
            HIPCHK(hipMemsetAsync(p->d_fstatus, 0, 2 * sizeof(unsigned), p->stream));
            HIPCHK(hipMemsetAsync(p->d_petd, 0xFF, (size_t)p->ndays * p->npad * sizeof(float), p->stream));
        }
        if ((rc = encode_block(p, t0, t1 - t0, d_prcp, d_pet, nullptr, (long)p->n, p->stream, &ok))) return rc;
        if (!ok) {
            HIPCHK(hipMemset(p->d_fstatus, 0, sizeof(unsigned)));
            return fail(SMASHX_E_UNSUPPORTED, "forcing block [" + std::to_string(t0) + ", " + std::to_string(t1) + ") is not of the compact form "
                        "(prcp = k * factor with k < 65535 or one gap value; pet = daily * ratio(hour)): reset the layout to fp32 and send the forcing again");
        }
        mark_block(p, t0, t1, t0 == 0);
        return 0;
    }
    HIPCHK(hipMemcpy2DAsync(p->d_prcp + (size_t)t0 * p->npad, (size_t)p->npad * 4, d_prcp, (size_t)p->n * 4, (size_t)p->n * 4, t1 - t0, hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipMemcpy2DAsync(p->d_pet + (size_t)t0 * p->npad, (size_t)p->npad * 4, d_pet, (size_t)p->n * 4, (size_t)p->n * 4, t1 - t0, hipMemcpyDeviceToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    mark_block(p, t0, t1, false);
    return 0;
}

namespace {
// The weights the cost stage reads (d_wgauge): the caller's, with 0 for a gauge that has no qo >= 0 on the steps optimize_start_step ..
// nt.  Such a gauge counts exactly as if its weight were 0: no cost, no place in the median, no seed.  qo is formed
// as prepare_signature and sx_qo form it.  On a plan with median slots an empty gauge that holds a slot is refused: dropping it would
// change the slot count of the whole decomposition.  Nothing of the plan is changed.
bool gauge_has_data(const smashx_plan* p, const std::vector<float>& h_qobs, int g, int s0) {
    for (int t = s0; t < p->nt; ++t) {
        const float qo = h_qobs[(size_t)g * p->nt + t] * p->cfg.dt / ((float)p->gauge_flwacc_h[g] * p->cfg.dx * p->cfg.dx) * 1e3f;
        if (qo >= 0.f) return true;
    }
    return false;
}
// (smashx_set_median_slots is meant to come before the options; called after options and qobs it makes the same refusal itself)
int effective_wgauge(const smashx_plan* p, const std::vector<float>& w, const std::vector<float>& h_qobs, int s0, std::vector<float>& eff) {
    eff = w;
    for (int g = 0; g < p->ng; ++g) {
        if (!(w[g] > 0.f || w[g] < 0.f)) continue;
        if (gauge_has_data(p, h_qobs, g, s0)) continue;
        if (p->med_nslots > 0 && w[g] < 0.f && p->med_slot_h[g] >= 0)
            return fail(SMASHX_E_UNSUPPORTED, "gauge " + std::to_string(g + 1) + " holds a median slot and has no qobs >= 0 from optimize_start_step on: "
                        "it would leave the median; declare the slots without it (smashx_set_median_slots) and give it wgauge = 0");
        eff[g] = 0.f;
    }
    return 0;
}
}  // namespace

int smashx_set_qobs(smashx_plan* p, const float* qobs) {
    if (!p || (!qobs && p->ng > 0)) return fail(SMASHX_E_ARG, "null argument");
    int rc = set_device(p); if (rc) return rc;
    std::vector<float> tr((size_t)std::max(p->ng, 1) * p->nt);
    for (int g = 0; g < p->ng; ++g)
        for (int t = 0; t < p->nt; ++t) tr[(size_t)g * p->nt + t] = qobs[g + (size_t)p->ng * t];   // (ng,nt) column-major -> [g][t]
    if (!p->have_qobs || tr != p->h_qobs) {      // (the same observations again leave the effective weights as they are)
        std::vector<float> eff;
        if ((rc = effective_wgauge(p, p->wgauge, tr, p->opt.optimize_start_step - 1, eff))) return rc;
        HIPCHK(hipMemcpy(p->d_wgauge, eff.data(), eff.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(p->d_qobs, tr.data(), tr.size() * 4, hipMemcpyHostToDevice));
    p->have_qobs = true;
    if (tr != p->h_qobs) {          // (the drop-ins hand the same observations over before every call: nothing of the criteria's is redone then)
        p->h_qobs.swap(tr);
        p->sig.ready = false; p->sig.obs_s0 = -1;
    }
    return 0;
}

namespace {
// The signature criteria of options o on the plan's qobs and signature inputs (include/smashx_signature.h): refuses what the reference
// would compute from an unassigned num / den, builds the event tables of the slice that starts at optimize_start_step, and forms the
// quantiles of the observed series on the device.  Touches nothing of the plan but p->sig.
int prepare_signature(smashx_plan* p, const smashx_options* o, const std::vector<float>& wgauge) {
    auto& G = p->sig;
    G.a.want = 0; G.ready = false;
    bool crc = false, ev = false, erc = false, pct = false;
    for (int j = 0; j < o->njf; ++j) {
        const int f = o->jobs_fun[j];
        crc |= f == SMASHX_CRC; erc |= f == SMASHX_ERC; pct |= f >= SMASHX_CFP2 && f <= SMASHX_CFP90;
        ev |= f == SMASHX_EPF || f == SMASHX_ELT || f == SMASHX_ERC;
    }
    if (!(crc || ev || pct) || p->ng == 0) return 0;
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "signature-based jobs_fun on a tiled plan (tile / owner_mask)");
    if (!G.have) return fail(SMASHX_E_UNSUPPORTED, "signature-based jobs_fun read mean_prcp: call smashx_set_signature_inputs first");
    if (ev && !G.have_mask) return fail(SMASHX_E_UNSUPPORTED, "Epf / Elt / Erc read mask_event: smashx_set_signature_inputs was given none");
    if (!p->have_qobs) return fail(SMASHX_E_STATE, "signature-based jobs_fun: set qobs before the options");
    const int nt = p->nt, ng = p->ng, s0 = o->optimize_start_step - 1;
    std::vector<int> flw(ng);
    HIPCHK(hipMemcpy(flw.data(), p->d_gauge_flwacc, (size_t)ng * 4, hipMemcpyDeviceToHost));
    std::vector<int> nev(ng, 0);
    std::vector<std::vector<int>> evs(ng);
    int maxev = 0;
    for (int g = 0; g < ng; ++g) {
        const float* po = &G.h_po[(size_t)g * nt];
        std::vector<char> valid(nt, 0);             // qo >= 0 and po >= 0 (mwd_cost.f90:847, 927)
        bool any = false;
        for (int t = s0; t < nt; ++t) {
            const float qo = p->h_qobs[(size_t)g * nt + t] * p->cfg.dt / ((float)flw[g] * p->cfg.dx * p->cfg.dx) * 1e3f;
            any |= qo >= 0.f;
            valid[t] = qo >= 0.f && po[t] >= 0.f;
        }
        const bool live = (wgauge[g] > 0.f || wgauge[g] < 0.f) && any;
        auto sum_po = [&](int a, int cnt) { float s = 0.f; for (int t = a; t < a + cnt; ++t) if (valid[t]) s = s + po[t]; return s; };
        if (crc && live && !(sum_po(s0, nt - s0) > 0.f))
            return fail(SMASHX_E_UNSUPPORTED, "Crc at gauge " + std::to_string(g + 1) + ": no precipitation > 0 on the steps with qobs >= 0 and mean_prcp >= 0; "
                        "the reference then reads a ratio it never assigned (mwd_cost.f90:937-964)");
        if (!ev) continue;
        const int* mk = &G.h_mask[(size_t)g * nt];
        for (int t = nt - 1; t >= s0; --t) if (mk[t] > 0) { nev[g] = mk[t]; break; }      // n_event = the last positive entry (:805-814)
        evs[g].assign((size_t)2 * nev[g], 0);
        for (int t = nt - 1; t >= s0; --t) if (mk[t] >= 1 && mk[t] <= nev[g]) { evs[g][2 * (mk[t] - 1)] = t; evs[g][2 * (mk[t] - 1) + 1]++; }
        maxev = std::max(maxev, nev[g]);
        if (erc && live) {
            bool assigned = false;
            for (int i = 0; i < nev[g] && !assigned; ++i) {
                if (sum_po(evs[g][2 * i], evs[g][2 * i + 1]) > 0.f) assigned = true;
                else return fail(SMASHX_E_UNSUPPORTED, "Erc at gauge " + std::to_string(g + 1) + ", event " + std::to_string(i + 1) + ": no precipitation > 0 on its valid "
                                 "steps and no earlier event assigned the ratio; the reference then reads it unassigned (mwd_cost.f90:890-905)");
            }
        }
    }
    if (ev) {
        if (maxev > G.maxev_cap) {
            p->dfree(G.d_ev); p->dfree(G.a.evres); p->dfree(G.a.evcoef); p->dfree(G.a.evden); p->dfree(G.a.evflag);
            G.d_ev = nullptr; G.a.evres = nullptr; G.a.evcoef = nullptr; G.a.evden = nullptr; G.a.evflag = nullptr; G.maxev_cap = -1;
            int rc;
            if ((rc = p->dmalloc(&G.d_ev, (size_t)ng * maxev * 2))) return rc;
            if ((rc = p->dmalloc(&G.a.evres, (size_t)ng * maxev))) return rc;
            if ((rc = p->dmalloc(&G.a.evcoef, (size_t)ng * SX_MAXJF * maxev))) return rc;
            if ((rc = p->dmalloc(&G.a.evden, (size_t)maxev))) return rc;
            if ((rc = p->dmalloc(&G.a.evflag, (size_t)maxev))) return rc;
            G.maxev_cap = maxev;
        }
        std::vector<int> tab((size_t)std::max(1, ng * maxev * 2), 0);
        for (int g = 0; g < ng; ++g) std::copy(evs[g].begin(), evs[g].end(), tab.begin() + (size_t)g * maxev * 2);
        HIPCHK(hipMemcpy(G.d_ev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(G.d_nev, nev.data(), (size_t)ng * 4, hipMemcpyHostToDevice));
    }
    G.a.po = G.d_po; G.a.nev = G.d_nev; G.a.ev = G.d_ev; G.a.maxev = maxev;
    G.a.lds = 0;
    { const char* e = getenv("SMASHX_SIG_REPLAY"); G.a.replay = (e && atoi(e) != 0) ? 1 : 0; }
    if (pct) {
        // the sort buffers of a gauge in LDS when the device grants them (8 B per step of the slice), else in the plan's scratch
        const size_t need = (size_t)(nt - s0) * 8;
        int lim = 0, dev = 0;
        const char* force = getenv("SMASHX_SIG_LDS");          // SMASHX_SIG_LDS=0: sort in the plan's scratch whatever the length (tests)
        if (force && atoi(force) == 0) { /* scratch */ }
        else if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && need <= (size_t)lim) {
            G.a.lds = 1;
            if (need > 48 * 1024)
                for (const void* k : {(const void*)sx_k_sig_pct, (const void*)sx_k_sig_obs})
                    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need) != hipSuccess) { (void)hipGetLastError(); G.a.lds = 0; }
        } else (void)hipGetLastError();
        if (!G.a.lds && !G.a.skey) {
            int rc;
            if ((rc = p->dmalloc(&G.a.skey, (size_t)ng * nt))) return rc;
            if ((rc = p->dmalloc(&G.a.sidx, (size_t)ng * nt))) return rc;
        }
        if (G.obs_s0 != s0 || G.obs_lds != G.a.lds) {
            // the quantiles of the observed series: they depend on qobs and the start step alone, so a calibration loop that sets the
            // same options before every sweep forms them once
            SxCostArgs C = cost_args(p, 0.f);
            C.s0 = s0; C.sig = G.a;
            hipLaunchKernelGGL(sx_k_sig_obs, dim3(ng), dim3(64), G.a.lds ? need : 0, p->stream_r, C);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(p->stream_r));
            G.obs_s0 = s0; G.obs_lds = G.a.lds;
        }
    }
    G.a.want = (crc ? SX_SIG_WANT_CRC : 0u) | (ev ? SX_SIG_WANT_EVENTS : 0u) | (pct ? SX_SIG_WANT_PCT : 0u);
    G.ready = true;
    return 0;
}
}  // namespace

int smashx_jobs_of_qsim(smashx_plan* p, const float* qsim, float jobs_b, float* jobs, float* qsim_b, const float* qsim_d, float* jobs_d) {
    if (!p || !qsim || !jobs || (qsim_d && !jobs_d)) return fail(SMASHX_E_ARG, "null argument");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_jobs_of_qsim: a tiled plan (tile / owner_mask) is not supported");
    int rc = set_device(p); if (rc) return rc;
    const int ng = p->ng, nt = p->nt;
    *jobs = 0.f; if (jobs_d) *jobs_d = 0.f;
    if (ng == 0) return 0;
    if (!p->have_qobs) return fail(SMASHX_E_STATE, "smashx_jobs_of_qsim: qobs not set");
    if ((rc = signature_state(p))) return rc;
    std::vector<char> seen(std::max(p->ngc, 1), 0);
    for (int g = 0; g < ng; ++g) {
        if (seen[p->gauge_gid[g]]) return fail(SMASHX_E_ARG, "smashx_jobs_of_qsim: two gauges share a cell, whose series cannot be prescribed twice");
        seen[p->gauge_gid[g]] = 1;
    }
    auto& G = p->sig;
    const size_t nq = (size_t)std::max(p->ngc, 1) * nt;
    if (!G.d_probe_b) {
        if ((rc = p->dmalloc(&G.d_probe_b, (size_t)ng * nt))) return rc;
        if ((rc = p->dmalloc(&G.d_probe_gb, nq))) return rc;
        if ((rc = p->dmalloc(&G.d_probe_gd, nq))) return rc;
        if ((rc = p->dmalloc(&G.d_probe_keep, nq + 4))) return rc;
    }
    std::vector<float> rows(nq, 0.f);
    auto to_rows = [&](const float* a) {
        for (int g = 0; g < ng; ++g)
            for (int t = 0; t < nt; ++t) rows[(size_t)p->gauge_gid[g] * nt + t] = a[g + (size_t)ng * t];      // (ng,nt) column-major -> [cell][t]
    };
    hipStream_t sR = p->stream_r;
    // what the last sweep left -- its gauge discharges and its cost -- is put aside and put back at the end
    HIPCHK(hipMemcpyAsync(G.d_probe_keep, p->A.qg, nq * 4, hipMemcpyDeviceToDevice, sR));
    HIPCHK(hipMemcpyAsync(G.d_probe_keep + nq, p->d_cost_out, 4 * 4, hipMemcpyDeviceToDevice, sR));
    to_rows(qsim);
    HIPCHK(hipMemcpyAsync(p->A.qg, rows.data(), nq * 4, hipMemcpyHostToDevice, sR));
    HIPCHK(hipStreamSynchronize(sR));
    p->launches.clear(); p->pool_used = 0;
    if ((rc = run_cost(p, qsim_b ? 1 : 0, jobs_b, G.d_probe_b, G.d_probe_gb))) return rc;
    if (qsim_d) {
        to_rows(qsim_d);
        HIPCHK(hipMemcpyAsync(G.d_probe_gd, rows.data(), nq * 4, hipMemcpyHostToDevice, sR));
        SxCostArgs C = cost_args(p, 0.f);
        hipLaunchKernelGGL(sx_k_cost_tangent, dim3(1), dim3(64), 0, sR, C, G.d_probe_gd, p->d_cost_out + 1);
        HIPCHK(hipMemcpyAsync(jobs_d, p->d_cost_out + 1, sizeof(float), hipMemcpyDeviceToHost, sR));
    }
    HIPCHK(hipMemcpyAsync(jobs, p->d_cost_out, sizeof(float), hipMemcpyDeviceToHost, sR));
    HIPCHK(hipMemcpyAsync(p->A.qg, G.d_probe_keep, nq * 4, hipMemcpyDeviceToDevice, sR));
    HIPCHK(hipMemcpyAsync(p->d_cost_out, G.d_probe_keep + nq, 4 * 4, hipMemcpyDeviceToDevice, sR));
    HIPCHK(hipStreamSynchronize(sR));
    HIPCHK(hipGetLastError());
    if (qsim_b) {
        std::vector<float> qb((size_t)ng * nt);
        HIPCHK(hipMemcpy(qb.data(), G.d_probe_b, qb.size() * 4, hipMemcpyDeviceToHost));
        for (int g = 0; g < ng; ++g)
            for (int t = 0; t < nt; ++t) qsim_b[g + (size_t)ng * t] = qb[(size_t)g * nt + t];
    }
    return 0;
}

int smashx_set_signature_inputs(smashx_plan* p, const float* mean_prcp, const int* mask_event) {
    if (!p) return fail(SMASHX_E_ARG, "null argument");
    if (p->ng == 0) return 0;
    if (!mean_prcp) return fail(SMASHX_E_ARG, "smashx_set_signature_inputs: mean_prcp is NULL");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_set_signature_inputs: a tiled plan (tile / owner_mask) is not supported: the criteria are sequential sums over a gauge's whole series");
    int rc = set_device(p); if (rc) return rc;
    const int ng = p->ng, nt = p->nt;
    auto& G = p->sig;
    std::vector<float> po((size_t)ng * nt);
    std::vector<int> mk;
    for (int g = 0; g < ng; ++g)
        for (int t = 0; t < nt; ++t) po[(size_t)g * nt + t] = mean_prcp[g + (size_t)ng * t];       // (ng,nt) column-major -> [g][t]
    if (mask_event) {
        mk.resize((size_t)ng * nt);
        for (int g = 0; g < ng; ++g)
            for (int t = 0; t < nt; ++t) {
                const int m = mask_event[g + (size_t)ng * t];
                if (m < 0 || m > nt) return fail(SMASHX_E_ARG, "smashx_set_signature_inputs: mask_event holds " + std::to_string(m) + " (0 outside events, 1..n inside, n <= ntime_step)");
                mk[(size_t)g * nt + t] = m;
            }
    }
    G.ready = false;
    if (!G.d_po) {
        if ((rc = p->dmalloc(&G.d_po, (size_t)ng * nt))) return rc;
        if ((rc = p->dmalloc(&G.d_nev, (size_t)ng))) return rc;
        if ((rc = p->dmalloc(&G.a.crc, (size_t)ng * 3))) return rc;
        if ((rc = p->dmalloc(&G.a.pct, (size_t)ng * 4))) return rc;
        if ((rc = p->dmalloc(&G.a.den_obs, (size_t)ng * 4))) return rc;
        if ((rc = p->dmalloc(&G.a.n_obs, (size_t)ng))) return rc;
    }
    if (G.have && po == G.h_po && mk == G.h_mask && G.have_mask == (mask_event != nullptr)) return 0;     // the same inputs again: nothing changes
    HIPCHK(hipMemcpy(G.d_po, po.data(), po.size() * 4, hipMemcpyHostToDevice));
    G.h_po.swap(po); G.h_mask.swap(mk);
    G.have = true; G.have_mask = mask_event != nullptr;
    return 0;
}

int smashx_set_options(smashx_plan* p, const smashx_options* o) {
    if (!p || !o) return fail(SMASHX_E_ARG, "null argument");
    int rc = set_device(p); if (rc) return rc;
    if (o->njf < 0 || o->njf > SX_MAXJF || o->njr < 0 || o->njr > 4) return fail(SMASHX_E_ARG, "njf/njr out of range");
    if (o->optimize_start_step < 1 || o->optimize_start_step > p->nt) return fail(SMASHX_E_ARG, "optimize_start_step out of range");
    for (int j = 0; j < o->njf; ++j)
        if (o->jobs_fun[j] < SMASHX_NSE || o->jobs_fun[j] > SMASHX_ERC)
            return fail(SMASHX_E_UNSUPPORTED, "unknown jobs_fun (mwd_cost.f90:98-131)");
    for (int j = 0; j < o->njr; ++j)
        if (o->jreg_fun[j] < SMASHX_PRIOR || o->jreg_fun[j] > SMASHX_HARD_SMOOTHING)
            return fail(SMASHX_E_UNSUPPORTED, "unknown jreg_fun (prior / smoothing / hard_smoothing, mwd_cost.f90:199-224)");
    std::vector<float> eff;
    {   // the signature criteria and the gauges without data first: a refusal leaves the plan's options as they were, without the criteria's tables (run_cost checks)
        std::vector<float> w(std::max(p->ng, 1), 0.f);
        for (int g = 0; g < p->ng; ++g) w[g] = o->wgauge ? o->wgauge[g] : 1.f / p->ng;
        if ((rc = prepare_signature(p, o, w))) return rc;
        if (p->have_qobs && (rc = effective_wgauge(p, w, p->h_qobs, o->optimize_start_step - 1, eff))) return rc;
    }
    p->opt = *o;
    p->jr_ready = false;
    p->opt.wgauge = nullptr;
    for (int g = 0; g < p->ng; ++g) {
        const float w = o->wgauge ? o->wgauge[g] : 1.f / p->ng;
        if (w < 0.f && p->tiled && p->med_nslots == 0)
            return fail(SMASHX_E_UNSUPPORTED, "negative wgauge (median over gauges) on a tiled plan: declare the slots of the whole decomposition first (smashx_set_median_slots)");
        if (p->med_nslots > 0 && (w < 0.f) != (p->med_slot_h[g] >= 0))
            return fail(SMASHX_E_ARG, "smashx_set_median_slots and wgauge disagree: exactly the negative-weight gauges have a slot");
        p->wgauge[g] = w;
    }
    if (!p->have_qobs) eff = p->wgauge;
    HIPCHK(hipMemcpy(p->d_wgauge, eff.data(), eff.size() * 4, hipMemcpyHostToDevice));
    p->have_options = true;
    p->hyp.options = true;
    return 0;
}

namespace {
// compute_jreg (and COMPUTE_JREG_B when adjoint) on the regularisation stream: independent of the simulation
int run_jreg(smashx_plan* p, int adjoint, float cost_b) {
    if (!p->jr_ready) return fail(SMASHX_E_STATE, "jreg is on but the current upload carried no background fields");
    hipStream_t sJ = p->stream_j;
    const dim3 b(256), gfull((unsigned)((p->n2 + 255) / 256));
    const int nrow = p->cfg.nrow, ncol = p->cfg.ncol;
    SxJregChains& ch = p->jchains;
    ch.nchain = 2 * p->opt.njr;
    long planes = 0;
    for (int i = 0; i < p->opt.njr; ++i)
        for (int grp = 0; grp < 2; ++grp) {
            const int c = 2 * i + grp, lo = grp ? SMASHX_GNP : 0, hi = grp ? SMASHX_GNP + SMASHX_GNS : SMASHX_GNP;
            ch.first[c] = planes; ch.nplane[c] = 0;
            for (int idx = lo; idx < hi; ++idx) if (jreg_optim(p, idx) > 0) { ch.nplane[c]++; planes++; }
        }
    if ((size_t)planes > p->jterm_planes) {
        int rc = p->dmalloc(&p->d_jterm, (size_t)planes * p->n2); if (rc) return rc;   // (the smaller buffer stays owned by the plan)
        p->jterm_planes = (size_t)planes;
    }
    for (int i = 0; i < p->opt.njr; ++i)
        for (int grp = 0; grp < 2; ++grp) {
            const int c = 2 * i + grp, lo = grp ? SMASHX_GNP : 0, hi = grp ? SMASHX_GNP + SMASHX_GNS : SMASHX_GNP;
            long slot = ch.first[c];
            for (int idx = lo; idx < hi; ++idx) {
                if (jreg_optim(p, idx) <= 0) continue;
                float* t = p->d_jterm + (size_t)slot++ * p->n2;
                if (p->opt.jreg_fun[i] == SMASHX_PRIOR)
                    hipLaunchKernelGGL(sx_k_prior_terms, gfull, b, 0, sJ, t, p->d_jx[idx], p->d_jb[idx], p->n2);
                else
                    hipLaunchKernelGGL(sx_k_smooth_terms, gfull, b, 0, sJ, t, p->d_jx[idx], p->d_jb[idx],
                                       p->opt.jreg_fun[i] == SMASHX_SMOOTHING ? 1 : 0, p->d_active, nrow, ncol);
            }
        }
    hipLaunchKernelGGL(sx_k_seq_sum, dim3(ch.nchain), dim3(64), 0, sJ, p->d_jterm, ch, p->n2, p->d_jsum);
    if (adjoint) {
        const float jreg_b = p->opt.wjreg * cost_b;                       // COMPUTE_COST_B: cost = jobs + wjreg * jreg
        for (int idx = 0; idx < SMASHX_GNP + SMASHX_GNS; ++idx)
            if (jreg_optim(p, idx) > 0) HIPCHK(hipMemsetAsync(p->d_jg[idx], 0, (size_t)p->n2 * 4, sJ));
        for (int i = p->opt.njr - 1; i >= 0; --i) {
            const float w = p->opt.wjreg_fun[i];
            const bool prior = p->opt.jreg_fun[i] == SMASHX_PRIOR;
            const float res_b = prior ? w * jreg_b : (w * w) * jreg_b;    // wjreg_fun(i)**2 for the smoothing terms
            for (int idx = SMASHX_GNP + SMASHX_GNS - 1; idx >= 0; --idx) {
                if (jreg_optim(p, idx) <= 0) continue;
                if (prior) hipLaunchKernelGGL(sx_k_prior_b, gfull, b, 0, sJ, p->d_jg[idx], p->d_jx[idx], p->d_jb[idx], res_b, p->n2);
                else hipLaunchKernelGGL(sx_k_smooth_b, gfull, b, 0, sJ, p->d_jg[idx], p->d_jx[idx], p->d_jb[idx],
                                        p->opt.jreg_fun[i] == SMASHX_SMOOTHING ? 1 : 0, p->d_active, nrow, ncol, res_b);
            }
        }
        if (p->opt.denormalize_forward)
            for (int idx = 0; idx < SMASHX_GNP + SMASHX_GNS; ++idx)
                if (jreg_optim(p, idx) > 0) hipLaunchKernelGGL(sx_k_plane_div, gfull, b, 0, sJ, p->d_jg[idx], jreg_span(p, idx), p->n2);
    }
    HIPCHK(hipEventRecord(p->ev_j, sJ));
    return 0;
}
// the regulariser's total from the sums of its chains (or their tangents): weighted sums of the chains, then parameters + states
// (mwd_cost.f90:199-228; COMPUTE_JREG_D runs the same sums in the same order)
float jreg_total(const smashx_plan* p, const float* sums) {
    float pj = 0.f, sj = 0.f;
    for (int i = 0; i < p->opt.njr; ++i) {
        const float w = p->opt.wjreg_fun[i];
        const float ww = p->opt.jreg_fun[i] == SMASHX_PRIOR ? w : w * w;
        pj = pj + ww * sums[2 * i];
        sj = sj + ww * sums[2 * i + 1];
    }
    return pj + sj;
}
}  // namespace

int smashx_upload(smashx_plan* p, const smashx_parameters* params, const smashx_parameters* params_bgd,
                  const smashx_states* states, const smashx_states* states_bgd) {
    if (!p || !params || !states) return fail(SMASHX_E_ARG, "null argument");
    int rc = set_device(p); if (rc) return rc;
    const int st = p->st;
    const dim3 b(256), gfull((unsigned)((p->n2 + 255) / 256)), gk((p->n + 255) / 256);
    for (int s = 0; s < SX_NSLOTS; ++s) {
        const int f = sx_slot_field(st, s);
        if (f < 0) continue;
        const float* h = host_plane(params, states, f);
        if (!h) {     // NULL = unchanged since the last upload (calibration loops move only the optimised fields)
            if (!p->uploaded) return fail(SMASHX_E_ARG, sx_field_is_state(f) ? "a state field the structure uses is NULL" : "a parameter field the structure uses is NULL");
            continue;
        }
        HIPCHK(hipMemcpyAsync(p->d_full[f], h, (size_t)p->n2 * 4, hipMemcpyHostToDevice, p->stream));
        if (p->opt.denormalize_forward)
            hipLaunchKernelGGL(k_denormalize, gfull, b, 0, p->stream, p->d_full[f], p->n2, field_lb(p, f), field_ub(p, f));
        hipLaunchKernelGGL(k_gather, gk, b, 0, p->stream, slot_vecs(p, s).start, p->d_full[f], p->d_cell_flat, p->n);
    }
    hipLaunchKernelGGL(sx_k_prep_routing, gk, b, 0, p->stream, p->A);
    p->jr_ready = false;
    if (p->opt.njr > 0) {
        // compute_jreg reads the control vector as compute_cost holds it: normalised again after the forward run
        // when denormalize_forward is set (mwd_cost.f90:284-291), plus the background fields
        if (!params_bgd || !states_bgd) return fail(SMASHX_E_ARG, "jreg needs parameters_bgd and states_bgd");
        for (int idx = 0; idx < SMASHX_GNP + SMASHX_GNS; ++idx) {
            if (jreg_optim(p, idx) <= 0) continue;
            const float* h = host_plane(params, states, idx);
            const float* hb = host_plane(params_bgd, states_bgd, idx);
            if (!h || !hb) return fail(SMASHX_E_ARG, "an optimised field (optim_parameters / optim_states) or its background is NULL");
            if (!p->d_jx[idx]) {
                if ((rc = p->dmalloc(&p->d_jx[idx], (size_t)p->n2))) return rc;
                if ((rc = p->dmalloc(&p->d_jb[idx], (size_t)p->n2))) return rc;
                if ((rc = p->dmalloc(&p->d_jg[idx], (size_t)p->n2))) return rc;
            }
            const float lb = field_lb(p, idx), ub = field_ub(p, idx);
            HIPCHK(hipMemcpyAsync(p->d_jx[idx], h, (size_t)p->n2 * 4, hipMemcpyHostToDevice, p->stream));
            if (p->opt.denormalize_forward) {
                hipLaunchKernelGGL(k_denormalize, gfull, b, 0, p->stream, p->d_jx[idx], p->n2, lb, ub);
                hipLaunchKernelGGL(k_normalize, gfull, b, 0, p->stream, p->d_jx[idx], p->n2, lb, ub);
            }
            HIPCHK(hipMemcpyAsync(p->d_jb[idx], hb, (size_t)p->n2 * 4, hipMemcpyHostToDevice, p->stream));
        }
        p->jr_ready = true;
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    p->uploaded = true;
    return 0;
}

static int sweep_once(smashx_plan* p, int adjoint, float cost_b, bool* stalled_out);
static int close_forcing(smashx_plan* p) {       // compact PET: days that never showed a daytime hour take the value 0
    if (!p->petd_open || !p->d_petd) return 0;
    const size_t n = (size_t)p->ndays * p->npad;
    hipLaunchKernelGGL(k_close_petd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, p->d_petd, n);
    p->petd_open = false;
    return 0;
}

// A chained routing launch draws its groups by ticket (sx_kernels.h), so a group only waits for groups that are resident or done: every
// input from outside the launch (vertical kernel, round 0, series received from other ranks) is complete before the launch starts.
// Should a wait nevertheless exhaust its poll limit, a flag is raised and the sweep's results are void: the plan then drops to one launch per
// round for good and the sweep is run again; the ranks of a decomposition take that decision together (one all-reduce per sweep).
int smashx_sweep(smashx_plan* p, int adjoint, float cost_b) {
    bool stalled = false;
    int rc = sweep_once(p, adjoint, cost_b, &stalled);
    if (rc) return rc;
    const bool agree = p->xcomm != nullptr && p->chain;      // a decomposition decides together: same condition on every rank
    if (agree) {
        double v = stalled ? 1.0 : 0.0;
        if ((rc = smashx_comm_allreduce_sum(p->xcomm, &v, 1))) return rc;
        stalled = v > 0.0;
    }
    if (!stalled) return 0;
    if (p->halo_fn && !p->xcomm)     // host-callback exchange: the neighbours of a tile cannot be made to repeat their sweep from here
        return fail(SMASHX_E_HIP, "chained routing launch stalled waiting for an upstream group (results invalid); set SMASHX_CHAIN_ROUNDS=0");
    fprintf(stderr, "smashx: a chained routing launch stalled (poll limit reached); this plan now runs one launch per routing round%s\n",
            p->xcomm ? " (every rank of the decomposition does)" : "");
    p->chain = false;
    p->A.mute_group = -1;
    rc = sweep_once(p, adjoint, cost_b, &stalled);
    if (rc) return rc;
    return stalled ? fail(SMASHX_E_HIP, "routing stalled without chained rounds (internal error)") : 0;
}

// ---- boundary-series exchange of a tiled plan (used by the sweep and by the tangent model) ---------------------------------
// move the boundary series of one sub-chunk between the exchange rows (xarr: xT, or xdT for the tangents) and the message buffers
// (the caller's, or the plan's own in peer-grouped edge order when RCCL carries them)
static void sx_halo_move(smashx_plan* p, bool native, float* xarr, bool pack, bool out_edges, int off, int T, hipStream_t st) {
    const int nedge = out_edges ? p->n_out : p->n_in;
    if (nedge == 0) return;
    const int Tq = (T + 3) / 4;
    float4* x4 = reinterpret_cast<float4*>(xarr) + (size_t)(off / 4) * p->A.nx;
    float4* buf = reinterpret_cast<float4*>(native ? (out_edges ? p->x_out : p->x_in) : (out_edges ? p->halo_out : p->halo_in));
    const int* slots = native ? (out_edges ? p->d_out_xp : p->d_in_xp) : (out_edges ? p->d_out_x : p->d_in_x);
    const dim3 g((nedge * Tq + 255) / 256), b(256);
    if (pack) hipLaunchKernelGGL(k_halo_pack, g, b, 0, st, buf, x4, slots, nedge, p->A.nx, Tq);
    else hipLaunchKernelGGL(k_halo_unpack, g, b, 0, st, x4, buf, slots, nedge, p->A.nx, Tq);
}
// one grouped send or recv per sub-chunk: a message per peer = its edges x the sub-chunk's steps, stream-ordered on st
static int sx_halo_xfer(smashx_plan* p, bool send, bool out_edges, int T, hipStream_t st) {
    const std::vector<PeerSeg>& segs = out_edges ? p->out_segs : p->in_segs;
    if (segs.empty()) return 0;
    RcclApi& R = rccl();
    float* buf = out_edges ? p->x_out : p->x_in;
    const size_t per_edge = (size_t)((T + 3) / 4) * 4;
    static const bool trace = getenv("SMASHX_TRACE_XFER") != nullptr;     // debugging aid: one line per posted group, completion awaited
    if (trace) {
        std::string peers;
        for (const PeerSeg& sg : segs) peers += " " + std::to_string(sg.rank) + ":" + std::to_string(sg.count);
        fprintf(stderr, "[smashx rank %d] %s %s edges, %d steps, peers(rank:edges)%s\n", p->xcomm->rank, send ? "send" : "recv",
                out_edges ? "out" : "in", T, peers.c_str());
    }
    NCCLCHK(R.GroupStart());
    for (const PeerSeg& sg : segs) {
        float* b = buf + (size_t)sg.first * per_edge;
        const ncclResult_t r = send ? R.Send(b, (size_t)sg.count * per_edge, ncclFloat, sg.rank, p->xcomm->comm, st)
                                    : R.Recv(b, (size_t)sg.count * per_edge, ncclFloat, sg.rank, p->xcomm->comm, st);
        if (r != ncclSuccess) { (void)R.GroupEnd(); return fail(SMASHX_E_HIP, std::string("ncclSend/ncclRecv: ") + R.GetErrorString(r)); }
    }
    NCCLCHK(R.GroupEnd());
    if (trace) {
        HIPCHK(hipStreamSynchronize(st));
        fprintf(stderr, "[smashx rank %d]   ... completed\n", p->xcomm->rank);
    }
    return 0;
}
// phases as in smashx_halo_fn: 0 FWD_RECV (in), 1 FWD_SEND (out), 2 ADJ_RECV (out), 3 ADJ_SEND (in)
static int sx_halo_hook(smashx_plan* p, bool native, int phase, int t0, int T, hipStream_t st) {
    if (native) return sx_halo_xfer(p, phase == 1 || phase == 3, phase == 1 || phase == 2, T, st);
    // host callback: the packed buffer must be complete before the host moves it; the unpack of the previous message must have
    // consumed the receive buffer before the host fills it again
    HIPCHK(hipStreamSynchronize(st));
    const int rc2 = p->halo_fn(p->halo_user, phase, t0, T);
    return rc2 ? fail(SMASHX_E_ARG, "halo callback failed") : 0;
}

// ---- one sweep: its frame (sweep_begin / sweep_end), its parts on a small context, its schedule (sweep_once) --------------------
namespace {
// What every sweep over the period starts with (sweep_once, smashx_forward_d): no launch marked yet, the forcing closed, the R stream
// behind the V stream, the stall flag of the chained launches clear (diagnostics: and the four ints a stalled launch leaves behind it,
// which only sweep_once reports), the states back at the uploaded ones.
int sweep_begin(smashx_plan* p, bool diagnostics) {
    p->launches.clear(); p->pool_used = 0;
    int rc = close_forcing(p); if (rc) return rc;
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    HIPCHK(hipStreamWaitEvent(p->stream_r, p->ev0, 0));
    p->chain_used = false;
    HIPCHK(hipMemsetAsync(p->A.prog + p->sch.ngroups, 0, sizeof(int), p->stream_r));   // stall flag of the chained launches
    if (diagnostics) HIPCHK(hipMemsetAsync(p->A.prog + p->sch.ngroups + 3, 0, 4 * sizeof(int), p->stream_r));   // ... and its diagnostics
    return restore_states(p);
}
// ... and ends with: both streams drained, the launches' errors collected, the stall flag read if a chained launch ran
int sweep_end(smashx_plan* p, bool* stalled) {
    *stalled = false;
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipStreamSynchronize(p->stream_r));
    HIPCHK(hipGetLastError());
    if (p->chain_used) {
        int flag = 0;
        HIPCHK(hipMemcpy(&flag, p->A.prog + p->sch.ngroups, sizeof(int), hipMemcpyDeviceToHost));
        *stalled = flag != 0;
    }
    return 0;
}

struct Sweep {
    smashx_plan* p;
    hipStream_t sV, sR;
    int C;               // storage chunks
    bool native, halo;   // the exchange runs over RCCL; boundary series are exchanged at all
    bool keep_in;        // the inlet series of the chunks the reverse sweep recomputes are kept
    bool keep;           // kept chain tape
};
Sweep sweep_context(smashx_plan* p, bool adjoint) {
    Sweep S{p, p->stream, p->stream_r, p->nchunks, p->xcomm != nullptr, false, false, false};
    S.halo = (p->halo_fn || S.native) && (p->n_out > 0 || p->n_in > 0);
    // Recomputation of a storage chunk (reverse sweep) needs no neighbour: the inlet series a rank received for that chunk in the first
    // pass are kept (n_in edges x Tc steps x 4 B per chunk) and unpacked again, and nothing is sent -- the ranks downstream kept theirs.
    // A sweep then changes direction twice between the ranks (forward -> reverse) instead of twice per recomputed chunk more.
    S.keep_in = adjoint && S.halo && p->n_in > 0 && S.C > 1;
    // Kept chain tape: the chained launch of the storage chunks 0 .. C - 2 tapes in the FIRST pass (where it runs under the next chunk's
    // vertical kernel) into the plan's kept rows; their recomputation then needs neither the copy into the staging rows nor the chained
    // launch -- round 0 is upstream of it, gauge discharge and cost are known, the chunk-end states come from the checkpoints -- and
    // the chained adjoint launch reads the kept rows.
    S.keep = adjoint && S.C > 1 && p->hrk && !S.halo && chain_first(p) < p->sch.nrounds;
    return S;
}
int nsub_of(const smashx_plan* p, int T) { return (T + p->Tp - 1) / p->Tp; }
size_t keep_sub(const smashx_plan* p) { return (size_t)std::max(p->n_in, 1) * (size_t)((p->Tp + 3) / 4) * 4; }      // floats of one sub-chunk's message
float* kept_rows(const Sweep& S, int c) {
    smashx_plan* p = S.p;
    return (S.keep && c < S.C - 1) ? p->hrk + (size_t)c * (size_t)(p->Tc / 4) * (size_t)p->A.kncs * 4 : nullptr;
}
int ensure_inlet_keep(const Sweep& S) {
    smashx_plan* p = S.p;
    const size_t need = keep_sub(p) * nsub_of(p, p->Tc) * (size_t)(S.C - 1);
    if (!S.keep_in || p->x_keep_cap >= need) return 0;
    if (p->x_keep) p->dfree(p->x_keep);
    p->x_keep = nullptr; p->x_keep_cap = 0;
    int rc = p->dmalloc(&p->x_keep, need); if (rc) return rc;
    p->x_keep_cap = need;
    return 0;
}

// The exchange around the routing pass of sub-chunk jb of chunk c (exchange rows xarr: xT, or xdT for the tangents).  Inlet: the series
// of the in edges reach the exchange rows -- received (and kept), or taken from the first pass.  Outlet: the series of the out edges leave.
int inlet_series(const Sweep& S, float* xarr, int c, int jb, int off, int t0, int T, bool recompute) {
    smashx_plan* p = S.p;
    if (!S.halo || p->n_in == 0) return 0;
    float* msg = S.native ? p->x_in : p->halo_in;
    float* kept = (S.keep_in && c < S.C - 1) ? p->x_keep + ((size_t)c * nsub_of(p, p->Tc) + jb) * keep_sub(p) : nullptr;
    const size_t bytes = (size_t)p->n_in * (size_t)((T + 3) / 4) * 4 * sizeof(float);
    if (recompute && kept) {
        HIPCHK(hipMemcpyAsync(msg, kept, bytes, hipMemcpyDeviceToDevice, S.sR));
    } else {
        int rc = sx_halo_hook(p, S.native, 0, t0, T, S.sR); if (rc) return rc;      // the message buffer now holds the upstream tiles' series
        if (kept) HIPCHK(hipMemcpyAsync(kept, msg, bytes, hipMemcpyDeviceToDevice, S.sR));
    }
    sx_halo_move(p, S.native, xarr, false, false, off, T, S.sR);
    return 0;
}
int outlet_series(const Sweep& S, float* xarr, int off, int t0, int T) {
    smashx_plan* p = S.p;
    if (!S.halo || p->n_out == 0) return 0;
    sx_halo_move(p, S.native, xarr, true, true, off, T, S.sR);
    return sx_halo_hook(p, S.native, 1, t0, T, S.sR);
}

// forward over one storage chunk: V(j) on the V stream, R(j) on the R stream as soon as V(j) is done
// (before a storage chunk's buffers are overwritten the V stream waits for the R stream sub-chunk by sub-chunk: buf_free)
int forward_chunk(const Sweep& S, int c, bool tape, bool recompute = false) {
    smashx_plan* p = S.p;
    static const bool early_release = []() { const char* e = getenv("SMASHX_EARLY_RELEASE"); return !(e && e[0] == '0'); }();
    const int t0c = c * p->Tc, Tcur = chunk_len(p, c), ns = nsub_of(p, Tcur);
    std::vector<hipEvent_t> ev(ns);
    // every vertical sub-chunk is queued at once: they only depend on each other (state carry, stream order) and write
    // disjoint parts of the chunk buffers, so the V stream never waits for the host, which blocks in the halo hooks
    // of the routing pipeline below (tiles) -- the vertical work then hides the pipeline fill across tiles
    for (int jb = 0; jb < ns; ++jb) {
        const int off = jb * p->Tp, T = std::min(p->Tp, Tcur - off);
        // this part of the chunk buffers was last used by the R stream in the previous pass over them (the reverse sweep ends on
        // the V stream): wait for that sub-chunk only, so that the routing of chunk c's tail runs under chunk c + 1's first kernels
        if (jb < (int)p->buf_free.size() && p->buf_free[jb]) { HIPCHK(hipStreamWaitEvent(S.sV, p->buf_free[jb], 0)); p->buf_free[jb] = nullptr; }
        vert_fwd(p, off, tape, t0c + off, T);
        ev[jb] = p->event(); HIPCHK(hipEventRecord(ev[jb], S.sV));
    }
    for (int jb = 0; jb < ns; ++jb) {
        const int off = jb * p->Tp, T = std::min(p->Tp, Tcur - off);
        int rc = inlet_series(S, p->A.xT, c, jb, off, t0c + off, T, recompute); if (rc) return rc;
        HIPCHK(hipStreamWaitEvent(S.sR, ev[jb], 0));
        // The next pass over this part of the chunk buffers is a vertical kernel that overwrites qt (and, taped, the level tapes --
        // which no forward routing launch reads): it may start as soon as the routing has READ qt.  With the chained launch on staging
        // rows that is after round 0 and the copy pass -- the chained launch, a latency chain on a few CUs, then runs under the next
        // storage chunk's vertical kernel (first pass of a checkpointed sweep: 3 x 3.6 ms at 2048^2); else after the whole pass.
        if ((int)p->buf_free.size() <= jb) p->buf_free.resize(jb + 1, nullptr);
        p->buf_free[jb] = p->event();
        float* const hrk = kept_rows(S, c);
        route_fwd_rounds(p, off, tape, t0c + off, T, S.sR, 0, chain_first(p));
        const bool released = (hrk && recompute) ? false : route_fwd_chained(p, off, tape, t0c + off, T, S.sR, early_release ? p->buf_free[jb] : nullptr, hrk);
        if (!recompute && (rc = outlet_series(S, p->A.xT, off, t0c + off, T))) return rc;       // (a recomputed chunk sends nothing: every rank kept what it received)
        if (!released) HIPCHK(hipEventRecord(p->buf_free[jb], S.sR));
    }
    return 0;
}

// optional whole-domain stores (md_forward_structure.f90:158-194) of one storage chunk -> the caller's arrays
int export_domain(const Sweep& S, int c) {
    smashx_plan* p = S.p;
    const int t0c = c * p->Tc, Tcur = chunk_len(p, c);
    HIPCHK(hipStreamSynchronize(S.sV));
    HIPCHK(hipStreamSynchronize(S.sR));
    const long plane = p->dom_sparse ? p->n_sparse : p->n2;
    const int* idx = p->dom_sparse ? p->d_sparse_idx : p->d_cell_flat;
    const int nbmax = (int)std::max<long>(1, std::min<long>(p->stage_planes * p->n2 / plane, 1 << 15));
    for (int which = 0; which < 2; ++which) {
        float* host = which ? p->h_net_prcp_domain : p->h_qsim_domain;
        const float* src = which ? p->A.qtT : p->A.qdT;
        if (!host || !src) continue;
        for (int tl0 = 0; tl0 < Tcur; tl0 += nbmax) {
            const int nb = std::min(nbmax, Tcur - tl0);
            if (!p->dom_sparse || p->tiled)      // cells this plan does not write: inactive ones (dense form), other parts' (tiles)
                hipLaunchKernelGGL(k_fill, dim3((unsigned)(((size_t)nb * plane + 255) / 256)), dim3(256), 0, S.sV, p->d_stage, -99.f, (size_t)nb * plane);
            hipLaunchKernelGGL(k_domain_export, dim3((p->n + 255) / 256, nb), dim3(256), 0, S.sV, p->d_stage, src, idx, p->n, p->npad, plane, tl0, nb);
            HIPCHK(hipMemcpyAsync(host + (size_t)(t0c + tl0) * plane, p->d_stage, (size_t)nb * plane * 4, hipMemcpyDeviceToHost, S.sV));
            HIPCHK(hipStreamSynchronize(S.sV));
        }
    }
    return 0;
}

// gradient accumulators start from what COMPUTE_COST_B left in parameters_b / states_b: zero, or the
// regulariser's gradient for the optimised fields (forward_db.f90:10869-10874)
int seed_gradients(const Sweep& S) {
    smashx_plan* p = S.p;
    bool waited[2] = {false, false};     // a stream waits for the regulariser once
    for (const int s : SX_SEED_ORDER) {
        const bool on_r = sx_slot_on_routing(s);
        const int f = sx_slot_field(p->st, s);
        float* const g = slot_vecs(p, s).grad;
        HIPCHK(hipMemsetAsync(g, 0, (size_t)p->npad * 4, slot_stream(p, s)));
        if (p->opt.njr > 0 && f >= 0 && jreg_optim(p, f) > 0) {
            if (!waited[on_r]) { HIPCHK(hipStreamWaitEvent(slot_stream(p, s), p->ev_j, 0)); waited[on_r] = true; }
            hipLaunchKernelGGL(k_gather, dim3((p->n + 255) / 256), dim3(256), 0, slot_stream(p, s), g, p->d_jg[f], p->d_cell_flat, p->n);
        }
    }
    if (p->ng == 0) HIPCHK(hipMemsetAsync(p->A.qgb, 0, (size_t)std::max(p->ngc, 1) * p->nt * 4, S.sR));
    return 0;
}

// reverse over one storage chunk, recomputed first with the tape on unless it is the last one.  *adj_queued: the chained adjoint launch
// of this chunk is already on the R stream (in), that of the chunk below is (out)
int reverse_chunk(const Sweep& S, int c, bool* adj_queued) {
    smashx_plan* p = S.p;
    const int t0c = c * p->Tc, Tcur = chunk_len(p, c);
    int rc;
    if (c < S.C - 1) {
        if ((rc = restore_states(p, c))) return rc;
        if ((rc = forward_chunk(S, c, true, true))) return rc;
    }
    for (int jb = nsub_of(p, Tcur) - 1; jb >= 0; --jb) {
        const int off = jb * p->Tp, T = std::min(p->Tp, Tcur - off);
        if (S.halo && p->n_out > 0) {
            if ((rc = sx_halo_hook(p, S.native, 2, t0c + off, T, S.sR))) return rc;  // out_buf now holds the downstream tiles' adjoint contributions
            sx_halo_move(p, S.native, p->A.xT, false, true, off, T, S.sR);
        }
        route_adj_chained(p, off, t0c + off, T, S.sR, kept_rows(S, c), !*adj_queued, true);
        *adj_queued = false;
        route_adj_rounds(p, off, t0c + off, T, S.sR);
        hipEvent_t e = p->event();
        HIPCHK(hipEventRecord(e, S.sR));
        HIPCHK(hipStreamWaitEvent(S.sV, e, 0));
        // Early adjoint chain: the chained adjoint launch of the chunk below needs the kept tape, the cost seeds and the routing
        // carry this pass has just left -- nothing its recomputation produces -- and on staging rows it writes nothing the
        // vertical kernels or round 0 touch: queued here, it runs under this chunk's vertical adjoint and the recomputation's
        // vertical kernel.  Its copy out of the staging rows follows round 0 of the recomputation (stream order).
        if (jb == 0 && c > 0 && kept_rows(S, c - 1) && p->early_adj && p->chain && p->A.qsk) {
            route_adj_chained(p, 0, (c - 1) * p->Tc, chunk_len(p, c - 1), S.sR, kept_rows(S, c - 1), true, false);
            *adj_queued = true;
        }
        vert_adj(p, off, t0c + off, T);
        if (S.halo && p->n_in > 0) {
            sx_halo_move(p, S.native, p->A.xT, true, false, off, T, S.sR);
            if ((rc = sx_halo_hook(p, S.native, 3, t0c + off, T, S.sR))) return rc;
        }
    }
    return 0;
}

void report_stall(const smashx_plan* p) {
    int d[7] = {0};
    (void)hipMemcpy(d, p->A.prog + p->sch.ngroups, sizeof(d), hipMemcpyDeviceToHost);
    fprintf(stderr, "smashx: stall: group %d followed the progress of group %d, needed %d blocks, saw %d; tickets drawn %d, chained groups %d..%d, progress:",
            d[3] - 2, p->sch.ngroups + d[4], d[5], d[6], d[1], p->sch.round_group_begin[chain_first(p)], p->sch.ngroups - 1);
    std::vector<int> pr(p->sch.ngroups);
    (void)hipMemcpy(pr.data(), p->A.prog, pr.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (int g = p->sch.round_group_begin[chain_first(p)]; g < p->sch.ngroups; ++g) fprintf(stderr, " %d", pr[g]);
    fprintf(stderr, " (n_in %d n_out %d)\n", p->n_in, p->n_out);
}

void collect_timing(smashx_plan* p) {
    smashx_timing& tm = p->timing;
    std::memset(&tm, 0, sizeof(tm));
    (void)hipEventElapsedTime(&tm.sweep_ms, p->ev0, p->ev1);
    for (const Launch& l : p->launches) {
        float ms = 0.f;
        if (l.a && l.b) (void)hipEventElapsedTime(&ms, l.a, l.b);
        switch (l.kind) {
            case 0: tm.vert_fwd_ms += ms; tm.vert_fwd_launches++; tm.cellsteps[0] += l.cellsteps; break;
            case 1: tm.route_fwd_ms += ms; tm.route_fwd_launches++; tm.cellsteps[1] += l.cellsteps; break;
            case 2: tm.route_adj_ms += ms; tm.route_adj_launches++; tm.cellsteps[2] += l.cellsteps; break;
            case 3: tm.vert_adj_ms += ms; tm.vert_adj_launches++; tm.cellsteps[3] += l.cellsteps; break;
            case 5: tm.route_fwd_ms += ms; tm.route_fwd_launches++; tm.cellsteps[1] += l.cellsteps;
                    tm.route_fwd_chained_ms += ms; tm.route_fwd_chained_launches++; break;
            case 6: tm.route_adj_ms += ms; tm.route_adj_launches++; tm.cellsteps[2] += l.cellsteps;
                    tm.route_adj_chained_ms += ms; tm.route_adj_chained_launches++; break;
            case 7: tm.route_adj_ms += ms; tm.route_adj_chained_ms += ms; break;      // (the copy pass of a chained adjoint launch)
            default: tm.cost_ms += ms; break;
        }
    }
    tm.n_chunks = p->nchunks; tm.chunk_steps = p->Tc; tm.pipe_steps = p->Tp; tm.n_rounds = p->sch.nrounds; tm.n_groups = p->sch.ngroups;
    tm.device_bytes = p->bytes;
    tm.max_stage = p->sch.max_stage;
    tm.chain_staged = (p->chain && p->A.qsk != nullptr) ? 1 : 0;
    tm.n_chained_groups = chain_first(p) < p->sch.nrounds ? p->sch.ngroups - p->sch.round_group_begin[chain_first(p)] : 0;
}
}  // namespace

// The schedule of one sweep: first pass over the storage chunks (adjoint: a checkpoint before each, the tape on in the last), cost, then -- adjoint --
// the seeds and the reverse pass, last chunk first, every other chunk recomputed from its checkpoint.
static int sweep_once(smashx_plan* p, int adjoint, float cost_b, bool* stalled_out) {
    *stalled_out = false;
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
    if (!p->uploaded) return fail(SMASHX_E_STATE, "parameters/states not uploaded");
    int rc = signature_state(p); if (rc) return rc;
    if ((rc = set_device(p))) return rc;
    if ((rc = ensure_chunk_buffers(p, adjoint != 0))) return rc;
    if ((p->n_out > 0 || p->n_in > 0) && !p->halo_fn && !p->xcomm)
        return fail(SMASHX_E_STATE, "tile has boundary series but no exchange is set (smashx_set_exchange / smashx_set_halo)");
    p->buf_free.clear();             // (the previous sweep ended with both streams drained)
    if ((rc = sweep_begin(p, true))) return rc;
    if (p->opt.njr > 0) {
        HIPCHK(hipStreamWaitEvent(p->stream_j, p->ev0, 0));
        if ((rc = run_jreg(p, adjoint, cost_b))) return rc;
    }
    const Sweep S = sweep_context(p, adjoint != 0);
    if ((rc = ensure_inlet_keep(S))) return rc;
    p->dom_q_active = !adjoint && p->h_qsim_domain && p->A.qdT;
    if (!adjoint) {
        const bool dom = p->h_qsim_domain || p->h_net_prcp_domain;
        for (int c = 0; c < S.C; ++c) {
            if ((rc = forward_chunk(S, c, false))) return rc;
            if (dom && (rc = export_domain(S, c))) return rc;
        }
        if ((rc = run_cost(p, 0, 0.f))) return rc;
    } else {
        for (int c = 0; c < S.C; ++c) {
            if (S.C > 1 && (rc = checkpoint_states(p, c))) return rc;
            // the last storage chunk is the first one the reverse sweep needs: it runs with the tape on straight away and
            // is not recomputed
            if ((rc = forward_chunk(S, c, c == S.C - 1))) return rc;
        }
        if ((rc = run_cost(p, 1, cost_b))) return rc;
        if ((rc = seed_gradients(S))) return rc;
        bool adj_queued = false;
        for (int c = S.C - 1; c >= 0; --c)
            if ((rc = reverse_chunk(S, c, &adj_queued))) return rc;
    }
    {
        hipEvent_t e = p->event();
        HIPCHK(hipEventRecord(e, S.sR));
        HIPCHK(hipStreamWaitEvent(S.sV, e, 0));
    }
    HIPCHK(hipEventRecord(p->ev1, S.sV));
    if (p->opt.njr > 0) HIPCHK(hipStreamSynchronize(p->stream_j));
    if ((rc = sweep_end(p, stalled_out))) return rc;
    if (*stalled_out) {
        if (getenv("SMASHX_VERBOSE")) report_stall(p);
        return 0;
    }
    collect_timing(p);
    p->last_adjoint = adjoint;
    return 0;
}

// Output_DT%qsim_domain / net_prcp_domain (or their sparse_ forms): host arrays the next FORWARD sweeps fill
int smashx_set_domain_outputs(smashx_plan* p, float* qsim_domain, float* net_prcp_domain, int sparse) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (sparse && !p->d_sparse_idx && (qsim_domain || net_prcp_domain))
        return fail(SMASHX_E_ARG, "sparse domain outputs need mesh.path (the sparse cell numbering)");
    // a tiled plan fills the cells of its own part and leaves -99 everywhere else (the caller overlays the parts): dense form
    // (nrow, ncol, nt), or sparse form (nac, nt) with nac the WHOLE grid's active cells -- a part's cells keep their whole-grid numbers
    p->h_qsim_domain = qsim_domain; p->h_net_prcp_domain = net_prcp_domain; p->dom_sparse = sparse ? 1 : 0;
    return 0;
}

// diagnostics: start/end ticks (100 MHz wall clock) of every routing group in the last forward (pass 0) and
// adjoint (pass 1) routing launches; needs SMASHX_TRACE_GROUPS=1 at plan creation.  out: [2][ngroups][2].
int smashx_debug_group_times(smashx_plan* p, long long* out, int* round_of_group) {
    if (!p || !out) return fail(SMASHX_E_ARG, "null argument");
    if (!p->A.gtime) return fail(SMASHX_E_STATE, "group tracing is off (SMASHX_TRACE_GROUPS=1)");
    int rc = set_device(p); if (rc) return rc;
    HIPCHK(hipMemcpy(out, p->A.gtime, (size_t)4 * p->sch.ngroups * sizeof(long long), hipMemcpyDeviceToHost));
    if (round_of_group)
        for (int r = 0; r < p->sch.nrounds; ++r)
            for (int g = p->sch.round_group_begin[r]; g < p->sch.round_group_begin[r + 1]; ++g) round_of_group[g] = r;
    return 0;
}

// device self-test: counts calls where sx_fdiv (sx_math.h) differs from the IEEE quotient a/b for n pseudo-random
// operand pairs with b in [blo, bhi); out[0] = mismatches, out[1] = mismatches larger than one ulp.
int smashx_selftest_math(int device, long long n, unsigned seed, float blo, float bhi, long long* out) {
    if (!out || n <= 0) return fail(SMASHX_E_ARG, "bad argument");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_selftest_div, dim3(2048), dim3(256), 0, 0, (unsigned long long)n, seed, blo, bhi, d);
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SMASHX_E_HIP, hipGetErrorString(e));
    out[0] = (long long)h[0]; out[1] = (long long)h[1];
    return 0;
}

int smashx_selftest_paths(int device, long long n, unsigned seed, long long* out) {
    if (!out || n <= 0) return fail(SMASHX_E_ARG, "bad argument");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_selftest_paths, dim3(2048), dim3(256), 0, 0, (unsigned long long)n, seed, d);
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SMASHX_E_HIP, hipGetErrorString(e));
    out[0] = (long long)h[0]; out[1] = (long long)h[1];
    return 0;
}

int smashx_selftest_eval(int device, int fn, const float* x, const float* y, long long n, float* out0, float* out1) {
    const bool binary = fn == SMASHX_FN_POW || fn == SMASHX_FN_POWB || fn == SMASHX_FN_DIV || fn == SMASHX_FN_DIV4 ||
                        fn == SMASHX_FN_FDIV || fn == SMASHX_FN_DIV_FAST;
    const bool paired = fn == SMASHX_FN_POWB || fn == SMASHX_FN_POW_M4_M5 || fn == SMASHX_FN_POW_M025_M125 || fn == SMASHX_FN_POW_3P5_2P5;
    if (fn < 0 || fn >= SMASHX_FN_COUNT) return fail(SMASHX_E_ARG, "unknown math function id");
    if (!x || !out0 || (binary && !y) || (paired && !out1)) return fail(SMASHX_E_ARG, "null argument");
    if (n <= 0 || n > (1ll << 26) || (fn == SMASHX_FN_DIV4 && n % 4 != 0)) return fail(SMASHX_E_ARG, "n must be in [1, 2^26] (DIV4: a multiple of 4)");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    const size_t b = (size_t)n * sizeof(float);
    float *dx = nullptr, *dy = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipError_t e = hipMalloc((void**)&dx, b);
    if (e == hipSuccess) e = hipMalloc((void**)&d0, b);
    if (e == hipSuccess && binary) e = hipMalloc((void**)&dy, b);
    if (e == hipSuccess && paired) e = hipMalloc((void**)&d1, b);
    if (e == hipSuccess) e = hipMemcpy(dx, x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess && binary) e = hipMemcpy(dy, y, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const long long nt = fn == SMASHX_FN_DIV4 ? n / 4 : n;
        const unsigned grid = (unsigned)std::min<long long>((nt + 255) / 256, 8192);
        hipLaunchKernelGGL(k_selftest_eval, dim3(grid), dim3(256), 0, 0, fn, dx, dy, nt, d0, d1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out0, d0, b, hipMemcpyDeviceToHost);
    if (e == hipSuccess && paired) e = hipMemcpy(out1, d1, b, hipMemcpyDeviceToHost);
    (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(d0); (void)hipFree(d1);
    if (e != hipSuccess) return fail(SMASHX_E_HIP, hipGetErrorString(e));
    return 0;
}

int smashx_tile_probe(const smashx_config* cfg, const smashx_mesh* mesh, int* info, int* out_src, int* out_dst,
                      int* in_src, int* in_dst, int cap) {
    if (!cfg || !mesh || !info) return fail(SMASHX_E_ARG, "null argument");
    SxSchedule sch;
    const bool tiled = cfg->tile[1] > cfg->tile[0] && cfg->tile[3] > cfg->tile[2];
    const int M = cfg->group_size > 0 ? cfg->group_size : 512;
    const int rc = sx_build_schedule(cfg->nrow, cfg->ncol, mesh->flwdir, mesh->active_cell, cfg->ng, mesh->gauge_pos, M,
                                     tiled ? cfg->tile : nullptr, sch, mesh->owner_mask, sublevels_env());
    if (rc) return fail(rc == -5 ? SMASHX_E_MESH : SMASHX_E_ARG, sch.error);
    const int no = (int)sch.out_x.size(), ni = (int)sch.in_x.size();
    const int v[8] = {sch.n, sch.nrounds, sch.ngroups, sch.nslots, sch.nxslots, sch.max_stage, no, ni};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    if (no > cap || ni > cap) { if (out_src || in_src) return fail(SMASHX_E_ARG, "edge capacity too small"); return 0; }
    for (int i = 0; i < no; ++i) { if (out_src) out_src[i] = sch.out_src[i]; if (out_dst) out_dst[i] = sch.out_dst[i]; }
    for (int i = 0; i < ni; ++i) { if (in_src) in_src[i] = sch.in_src[i]; if (in_dst) in_dst[i] = sch.in_dst[i]; }
    return 0;
}

int smashx_halo_counts(const smashx_plan* p, int* n_out, int* n_in) {
    if (!p || !n_out || !n_in) return fail(SMASHX_E_ARG, "null argument");
    *n_out = p->n_out; *n_in = p->n_in;
    return 0;
}

int smashx_halo_edges(const smashx_plan* p, int* out_src, int* out_dst, int* in_src, int* in_dst) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    for (int i = 0; i < p->n_out; ++i) { if (out_src) out_src[i] = p->sch.out_src[i]; if (out_dst) out_dst[i] = p->sch.out_dst[i]; }
    for (int i = 0; i < p->n_in; ++i) { if (in_src) in_src[i] = p->sch.in_src[i]; if (in_dst) in_dst[i] = p->sch.in_dst[i]; }
    return 0;
}

int smashx_plan_chunking(smashx_plan* p, int* chunk_steps, int* pipe_steps) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    int rc = set_device(p); if (rc) return rc;
    if ((rc = ensure_chunk_buffers(p, true))) return rc;
    if (chunk_steps) *chunk_steps = p->Tc;
    if (pipe_steps) *pipe_steps = p->Tp;
    return 0;
}

// out = {free HBM when the storage-chunk length was chosen (bytes; -1 before that), total HBM of the device, bytes the plan holds now}
int smashx_plan_hbm(const smashx_plan* p, double out[3]) {
    if (!p || !out) return fail(SMASHX_E_ARG, "null argument");
    out[0] = p->hbm_free_at_plan; out[1] = p->hbm_total; out[2] = p->bytes;
    return 0;
}

int smashx_set_halo(smashx_plan* p, float* d_out_buf, float* d_in_buf, smashx_halo_fn fn, void* user) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (fn && ((p->n_out > 0 && !d_out_buf) || (p->n_in > 0 && !d_in_buf))) return fail(SMASHX_E_ARG, "halo buffers missing");
    p->halo_out = d_out_buf; p->halo_in = d_in_buf; p->halo_fn = fn; p->halo_user = user;
    return 0;
}

int smashx_set_median_slots(smashx_plan* p, int nslots, const int* slot_of_gauge, smashx_reduce_fn fn, void* user) {
    if (!p || nslots < 0 || (nslots > 0 && !slot_of_gauge)) return fail(SMASHX_E_ARG, "bad argument");
    int rc = set_device(p); if (rc) return rc;
    p->med_nslots = 0; p->med_fn = fn; p->med_user = user;
    if (nslots == 0) return 0;
    std::vector<int> sl(std::max(p->ng, 1), -1);
    for (int g = 0; g < p->ng; ++g) {
        sl[g] = slot_of_gauge[g];
        if (sl[g] < -1 || sl[g] >= nslots) return fail(SMASHX_E_ARG, "slot_of_gauge out of range");
    }
    if (p->have_qobs)      // after options and qobs: a slot for a negative-weight gauge without data is refused here as it is there
        for (int g = 0; g < p->ng; ++g) {
            if (!(p->wgauge[g] < 0.f) || sl[g] < 0 || gauge_has_data(p, p->h_qobs, g, p->opt.optimize_start_step - 1)) continue;
            return fail(SMASHX_E_UNSUPPORTED, "gauge " + std::to_string(g + 1) + " is given a median slot and has no qobs >= 0 from optimize_start_step on");
        }
    if (p->d_med_slot) { p->dfree(p->d_med_slot); p->dfree(p->d_medx); p->dfree(p->d_medx_idx); }
    if ((rc = p->upload_vec(&p->d_med_slot, sl))) return rc;
    p->med_slot_h = sl;
    if ((rc = p->dmalloc(&p->d_medx, (size_t)3 * nslots))) return rc;
    if ((rc = p->dmalloc(&p->d_medx_idx, (size_t)nslots))) return rc;
    p->med_nslots = nslots;
    return 0;
}

// ---- native exchange over RCCL -----------------------------------------------------------------------------------
int smashx_comm_unique_id(unsigned char id[SMASHX_COMM_ID_BYTES]) {
    if (!id) return fail(SMASHX_E_ARG, "null argument");
    RcclApi& R = rccl();
    if (!R.ok()) return fail(SMASHX_E_UNSUPPORTED, "RCCL unavailable: " + R.err);
    static_assert(sizeof(ncclUniqueId) == SMASHX_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    NCCLCHK(R.GetUniqueId(&u));
    std::memcpy(id, &u, sizeof(u));
    return 0;
}

int smashx_comm_create(const unsigned char id[SMASHX_COMM_ID_BYTES], int rank, int nranks, int device, void** comm) {
    if (!id || !comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(SMASHX_E_ARG, "bad argument");
    *comm = nullptr;
    RcclApi& R = rccl();
    if (!R.ok()) return fail(SMASHX_E_UNSUPPORTED, "RCCL unavailable: " + R.err);
    if (device >= 0) HIPCHK(hipSetDevice(device));
    SxComm* c = new SxComm();
    c->rank = rank; c->nranks = nranks; c->device = device;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclResult_t r = R.CommInitRank(&c->comm, nranks, u, rank);
    if (r != ncclSuccess) { delete c; return fail(SMASHX_E_HIP, std::string("ncclCommInitRank: ") + R.GetErrorString(r)); }
    if (hipStreamCreate(&c->stream) != hipSuccess || hipMalloc((void**)&c->d_buf, 64 * sizeof(double)) != hipSuccess) {
        (void)R.CommDestroy(c->comm); delete c; return fail(SMASHX_E_HIP, "hipStreamCreate / hipMalloc failed");
    }
    *comm = c;
    return 0;
}

static void smashx_forget_comm(smashx_plan* p, SxComm* c) { if (p->xcomm == c) p->xcomm = nullptr; }
// a plan leaves the list of the communicator it pointed to whenever that pointer changes (unset, switched, plan destroyed): a
// communicator's list only ever holds live plans that still use it
static void smashx_detach_plan(smashx_plan* p) {
    if (SxComm* c = p->xcomm) c->plans.erase(std::remove(c->plans.begin(), c->plans.end(), p), c->plans.end());
    p->xcomm = nullptr;
}

int smashx_comm_destroy(void* comm) {
    SxComm* c = (SxComm*)comm;
    if (!c) return 0;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    for (smashx_plan* q : c->plans) smashx_forget_comm(q, c);      // no plan keeps a pointer to a communicator that is gone
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (c->d_buf) (void)hipFree(c->d_buf);
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    delete c;
    return 0;
}

// what the communicator itself says about the run: ranks it spans (ncclCommCount) and the library's version code (ncclGetVersion)
int smashx_comm_info(void* comm, int* nranks, int* version) {
    SxComm* c = (SxComm*)comm;
    if (!c) return fail(SMASHX_E_ARG, "null communicator");
    RcclApi& R = rccl();
    int n = c->nranks, v = 0;
    if (R.CommCount) NCCLCHK(R.CommCount(c->comm, &n));
    if (R.GetVersion) NCCLCHK(R.GetVersion(&v));
    if (nranks) *nranks = n;
    if (version) *version = v;
    return 0;
}

int smashx_comm_allreduce_sum(void* comm, double* values, int n) {
    SxComm* c = (SxComm*)comm;
    if (!c || !values || n < 1 || n > 64) return fail(SMASHX_E_ARG, "bad argument (1 <= n <= 64)");
    if (c->device >= 0) HIPCHK(hipSetDevice(c->device));
    RcclApi& R = rccl();
    HIPCHK(hipMemcpyAsync(c->d_buf, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(R.AllReduce(c->d_buf, c->d_buf, (size_t)n, ncclDouble, ncclSum, c->comm, c->stream));
    HIPCHK(hipMemcpyAsync(values, c->d_buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int smashx_set_exchange(smashx_plan* p, void* comm, const int* out_peer, const int* in_peer) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    SxComm* c = (SxComm*)comm;
    if (!c) { smashx_detach_plan(p); return 0; }
    // The call is collective (an agreement all-reduce, then one grouped hello exchange): a rank that left early would leave its
    // neighbours waiting inside ncclGroupEnd for ever.  So everything that can fail locally -- argument checks, regrouping, allocations --
    // happens FIRST and only feeds a status word; the ranks then agree on the status together with the chunking, and enter the hello
    // group only if every rank reported success.
    int rc = 0, lrc = 0;
    std::string lerr;
    auto local = [&](int code, const std::string& msg) { if (!lrc) { lrc = code; lerr = msg; } };
    if ((p->n_out > 0 && !out_peer) || (p->n_in > 0 && !in_peer)) local(SMASHX_E_ARG, "peer lists missing");
    if ((rc = set_device(p))) return rc;            // (a wrong device id is a caller bug on this rank alone: nothing collective has started)
    if (!lrc && (rc = ensure_chunk_buffers(p, false))) local(rc, g_err);
    // regroup the boundary edges by peer rank; inside a peer they keep the order both sides share (sorted by source cell)
    std::vector<PeerSeg> out_segs, in_segs;
    std::vector<int> out_xp, in_xp;
    auto regroup = [&](int n, const int* peer, const std::vector<int>& xs, std::vector<PeerSeg>& segs, std::vector<int>& xp) {
        segs.clear();
        std::vector<int> order(n);
        xp.assign(std::max(n, 1), 0);
        for (int i = 0; i < n; ++i) {
            if (peer[i] < 0 || peer[i] >= c->nranks || peer[i] == c->rank) { local(SMASHX_E_ARG, "boundary edge with a bad peer rank"); return; }
            order[i] = i;
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return peer[a] < peer[b]; });
        for (int i = 0; i < n; ++i) {
            xp[i] = xs[order[i]];
            if (segs.empty() || segs.back().rank != peer[order[i]]) segs.push_back(PeerSeg{peer[order[i]], i, 0});
            segs.back().count++;
        }
    };
    if (!lrc) regroup(p->n_out, out_peer, p->sch.out_x, out_segs, out_xp);
    if (!lrc) regroup(p->n_in, in_peer, p->sch.in_x, in_segs, in_xp);
    int *d_oxp = nullptr, *d_ixp = nullptr;
    float* hello = nullptr;
    std::vector<int> peers;
    if (!lrc) {
        for (const PeerSeg& sg : out_segs) peers.push_back(sg.rank);
        for (const PeerSeg& sg : in_segs) if (std::find(peers.begin(), peers.end(), sg.rank) == peers.end()) peers.push_back(sg.rank);
        std::sort(peers.begin(), peers.end());
        if ((rc = p->upload_vec(&d_oxp, out_xp)) || (rc = p->upload_vec(&d_ixp, in_xp)) || (rc = p->dmalloc(&hello, 2 * std::max<size_t>(peers.size(), 1))))
            local(rc, g_err);
        if (!lrc && !p->x_out) {
            if ((rc = p->dmalloc(&p->x_out, (size_t)std::max(p->n_out, 1) * p->Tp)) || (rc = p->dmalloc(&p->x_in, (size_t)std::max(p->n_in, 1) * p->Tp)))
                local(rc, g_err);
        }
    }
    auto drop_new = [&]() { if (d_oxp) p->dfree(d_oxp); if (d_ixp) p->dfree(d_ixp); if (hello) p->dfree(hello); };
    // every rank must cut time identically (the messages are per pipeline sub-chunk), and every rank must have got this far
    {
        RcclApi& R = rccl();
        double v[7] = {(double)p->Tc, -(double)p->Tc, (double)p->Tp, -(double)p->Tp, (double)p->nt, -(double)p->nt, lrc ? 1.0 : 0.0};
        HIPCHK(hipMemcpyAsync(c->d_buf, v, sizeof(v), hipMemcpyHostToDevice, c->stream));
        NCCLCHK(R.AllReduce(c->d_buf, c->d_buf, 7, ncclDouble, ncclMax, c->comm, c->stream));
        HIPCHK(hipMemcpyAsync(v, c->d_buf, sizeof(v), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (lrc) { drop_new(); return fail(lrc, lerr); }
        if (v[6] != 0.0) { drop_new(); return fail(SMASHX_E_STATE, "smashx_set_exchange failed on another rank of the decomposition"); }
        if (v[0] != -v[1] || v[2] != -v[3] || v[4] != -v[5]) {
            drop_new();
            return fail(SMASHX_E_ARG, "the ranks of the decomposition disagree on chunk_steps / pipe_steps / nt (this rank: " +
                                      std::to_string(p->Tc) + " / " + std::to_string(p->Tp) + " / " + std::to_string(p->nt) + ")");
        }
    }
    // Connect now, symmetrically: RCCL sets a point-to-point connection up the first time a pair is used, inside ncclGroupEnd on the
    // HOST, and both ends must be inside a group naming each other at that moment.  During a sweep the ranks reach their groups in
    // dependency order (a tile only sends after it has received and routed), so first use there makes rank A wait for B's NEXT
    // group while B waits for A's current one (observed: 3 sub-catchment parts hang in their first sub-chunk).  Here every rank
    // exchanges one float with each neighbour in both directions within ONE group -- the all-to-all shape RCCL's schedule is built
    // for -- so no connection is ever set up inside a sweep.
    if (!peers.empty()) {
        RcclApi& R = rccl();
        HIPCHK(hipMemsetAsync(hello, 0, 2 * peers.size() * sizeof(float), c->stream));
        NCCLCHK(R.GroupStart());
        for (size_t i = 0; i < peers.size(); ++i) {
            ncclResult_t r1 = R.Send(hello + 2 * i, 1, ncclFloat, peers[i], c->comm, c->stream);
            ncclResult_t r2 = R.Recv(hello + 2 * i + 1, 1, ncclFloat, peers[i], c->comm, c->stream);
            if (r1 != ncclSuccess || r2 != ncclSuccess) { (void)R.GroupEnd(); return fail(SMASHX_E_HIP, "ncclSend/ncclRecv (connection set-up) failed"); }
        }
        NCCLCHK(R.GroupEnd());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    p->dfree(hello);
    if (p->d_out_xp) p->dfree(p->d_out_xp);          // a second call replaces the tables of the first
    if (p->d_in_xp) p->dfree(p->d_in_xp);
    p->d_out_xp = d_oxp; p->d_in_xp = d_ixp;
    p->out_segs.swap(out_segs); p->in_segs.swap(in_segs);
    if (p->xcomm != c) smashx_detach_plan(p);        // re-targeted: the previous communicator forgets this plan
    p->xcomm = c;
    if (std::find(c->plans.begin(), c->plans.end(), p) == c->plans.end()) c->plans.push_back(p);
    return 0;
}

// ---- control vector -----------------------------------------------------------------------------------------------------------
namespace {
int ctrl_fields(const smashx_plan* p, int* idx) {     // flagged fields the structure uses: parameters (0..15) then states (16..23)
    int nf = 0;
    for (int f = 0; f < SX_NFIELDS; ++f) if (jreg_optim(p, f) > 0) idx[nf++] = f;
    return nf;
}
int ctrl_prepare(smashx_plan* p, int nf) {
    int rc;
    if (!p->d_ctrl_pos) {
        // rank of every plan cell among the active cells in (col outer, row inner) order = ascending flat index row + col * nrow
        std::vector<int> order(p->n), pos(p->n);
        for (int k = 0; k < p->n; ++k) order[k] = k;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return p->sch.cell_flat[a] < p->sch.cell_flat[b]; });
        for (int i = 0; i < p->n; ++i) pos[order[i]] = i;
        if ((rc = p->upload_vec(&p->d_ctrl_pos, pos))) return rc;
    }
    const size_t need = (size_t)nf * p->n;
    if (need > p->ctrl_cap) {
        if (p->d_ctrl) p->dfree(p->d_ctrl);
        if ((rc = p->dmalloc(&p->d_ctrl, need))) return rc;
        p->ctrl_cap = need;
    }
    return 0;
}
struct CtrlField { float* cellv; float* full; float lb, ub; bool used; };
CtrlField ctrl_field(smashx_plan* p, int idx, bool grad) {
    CtrlField F{nullptr, nullptr, field_lb(p, idx), field_ub(p, idx), false};
    const int s = sx_field_slot(p->st, idx);
    if (s >= 0) { const SlotVecs V = slot_vecs(p, s); F.cellv = grad ? V.grad : V.start; F.full = p->d_full[idx]; F.used = true; }
    return F;
}
}  // namespace

int smashx_control_size(smashx_plan* p) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    int idx[SMASHX_GNP + SMASHX_GNS];
    return ctrl_fields(p, idx) * p->n;
}

int smashx_control_set(smashx_plan* p, const double* x) {
    if (!p || !x) return fail(SMASHX_E_ARG, "null argument");
    if (!p->uploaded) return fail(SMASHX_E_STATE, "smashx_control_set needs one complete smashx_upload first (the fields that are not optimised)");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "control vector on a tiled plan");
    int rc = set_device(p); if (rc) return rc;
    int idx[SMASHX_GNP + SMASHX_GNS];
    const int nf = ctrl_fields(p, idx);
    if (nf == 0) return fail(SMASHX_E_STATE, "no field is flagged in optim_parameters / optim_states");
    if ((rc = ctrl_prepare(p, nf))) return rc;
    HIPCHK(hipMemcpyAsync(p->d_ctrl, x, (size_t)nf * p->n * sizeof(double), hipMemcpyHostToDevice, p->stream));
    const dim3 b(256), gk((p->n + 255) / 256);
    for (int j = 0; j < nf; ++j) {
        const CtrlField F = ctrl_field(p, idx[j], false);
        float* jx = (p->opt.njr > 0 && p->d_jx[idx[j]]) ? p->d_jx[idx[j]] : nullptr;
        if (!F.used && !jx) continue;                // flagged but read by nothing: the reference carries it along, nothing here depends on it
        hipLaunchKernelGGL(k_control_set, gk, b, 0, p->stream, F.used ? F.cellv : nullptr, F.full, jx, p->d_ctrl, p->d_ctrl_pos, p->d_cell_flat,
                           p->n, (long)j * p->n, F.lb, F.ub, p->opt.denormalize_forward);
    }
    hipLaunchKernelGGL(sx_k_prep_routing, gk, b, 0, p->stream, p->A);
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

static int control_read(smashx_plan* p, double* x, int grad) {
    if (!p || !x) return fail(SMASHX_E_ARG, "null argument");
    if (!p->uploaded) return fail(SMASHX_E_STATE, "nothing uploaded");
    if (grad && !(p->adj_ready && p->last_adjoint)) return fail(SMASHX_E_STATE, "the last sweep was not an adjoint sweep");
    int rc = set_device(p); if (rc) return rc;
    int idx[SMASHX_GNP + SMASHX_GNS];
    const int nf = ctrl_fields(p, idx);
    if (nf == 0) return fail(SMASHX_E_STATE, "no field is flagged in optim_parameters / optim_states");
    if ((rc = ctrl_prepare(p, nf))) return rc;
    HIPCHK(hipMemsetAsync(p->d_ctrl, 0, (size_t)nf * p->n * sizeof(double), p->stream));
    const dim3 b(256), gk((p->n + 255) / 256);
    for (int j = 0; j < nf; ++j) {
        const CtrlField F = ctrl_field(p, idx[j], grad != 0);
        if (!F.used) {
            // a flagged field the structure does not read: only the regulariser knows it -- its plane (already in the optimiser's
            // space) or its gradient plane (COMPUTE_JREG_B, scaled like the download scales it)
            const float* plane = p->opt.njr > 0 ? (grad ? p->d_jg[idx[j]] : p->d_jx[idx[j]]) : nullptr;
            if (!plane) continue;
            hipLaunchKernelGGL(k_control_get, gk, b, 0, p->stream, p->d_ctrl, plane, p->d_ctrl_pos, p->d_cell_flat, p->n, (long)j * p->n,
                               F.lb, F.ub, grad ? p->opt.denormalize_forward : 0, grad, 1);
            continue;
        }
        hipLaunchKernelGGL(k_control_get, gk, b, 0, p->stream, p->d_ctrl, F.cellv, p->d_ctrl_pos, p->d_cell_flat, p->n, (long)j * p->n,
                           F.lb, F.ub, p->opt.denormalize_forward, grad, 0);
    }
    HIPCHK(hipMemcpyAsync(x, p->d_ctrl, (size_t)nf * p->n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    return 0;
}
int smashx_control_get(smashx_plan* p, double* x) { return control_read(p, x, 0); }
int smashx_control_gradient(smashx_plan* p, double* g) { return control_read(p, g, 1); }

int smashx_get_timing(const smashx_plan* p, smashx_timing* out) {
    if (!p || !out) return fail(SMASHX_E_ARG, "null argument");
    *out = p->timing;
    return 0;
}

int smashx_download(smashx_plan* p, int adjoint, smashx_parameters* params, smashx_states* states, float* qsim,
                    smashx_costs* costs, smashx_states* fstates, smashx_parameters* params_b, smashx_states* states_b) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    int rc = set_device(p); if (rc) return rc;
    const int st = p->st;
    const dim3 b(256), gfull((unsigned)((p->n2 + 255) / 256)), gk((p->n + 255) / 256);
    // discharge at gauges: output%qsim(ng,nt)
    if (qsim && p->ng > 0) {
        std::vector<float> qg((size_t)p->ngc * p->nt);
        HIPCHK(hipMemcpy(qg.data(), p->A.qg, qg.size() * 4, hipMemcpyDeviceToHost));
        for (int g = 0; g < p->ng; ++g)
            for (int t = 0; t < p->nt; ++t) qsim[g + (size_t)p->ng * t] = qg[(size_t)p->gauge_gid[g] * p->nt + t];
    }
    if (costs) {
        float jobs = 0.f;
        if (p->ng > 0) HIPCHK(hipMemcpy(&jobs, p->d_cost_out, 4, hipMemcpyDeviceToHost));
        float jreg = 0.f;
        if (p->opt.njr > 0) {
            float sums[SX_JREG_MAXCHAIN] = {0.f};
            HIPCHK(hipMemcpy(sums, p->d_jsum, sizeof(float) * 2 * p->opt.njr, hipMemcpyDeviceToHost));
            jreg = jreg_total(p, sums);
        }
        costs->cost = jobs + p->opt.wjreg * jreg;    // mwd_cost.f90:300
        costs->cost_jobs = jobs; costs->cost_jreg = jreg;
    }
    // final states: output%fstates = states (forward.f90:71); inactive cells keep their entry values
    if (fstates && !adjoint) {
        for (int s = SX_NPSLOTS; s < SX_NSLOTS; ++s) {
            const int f = sx_slot_field(st, s);
            float* const h = f < 0 ? nullptr : host_plane(nullptr, fstates, f);
            if (!h) continue;
            HIPCHK(hipMemcpyAsync(p->d_stage, p->d_full[f], (size_t)p->n2 * 4, hipMemcpyDeviceToDevice, p->stream));
            hipLaunchKernelGGL(k_scatter, gk, b, 0, p->stream, p->d_stage, slot_vecs(p, s).val, p->d_cell_flat, p->n, 1.f, 0);
            HIPCHK(hipMemcpyAsync(h, p->d_stage, (size_t)p->n2 * 4, hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipStreamSynchronize(p->stream));
        }
    }
    // parameters / states as the reference leaves them (forward.f90:33-38,72; mwd_cost.f90:284-298):
    // denormalised; base_forward additionally sends them through normalise -> denormalise inside compute_cost.
    if (p->opt.denormalize_forward) {
        bool touched = false;
        for (int s = 0; s < SX_NSLOTS; ++s) {
            const int f = sx_slot_field(st, s);
            float* const h = f < 0 ? nullptr : host_plane(params, states, f);
            if (!h) continue;
            touched = true;
            if (!adjoint) {
                hipLaunchKernelGGL(k_normalize, gfull, b, 0, p->stream, p->d_full[f], p->n2, field_lb(p, f), field_ub(p, f));
                hipLaunchKernelGGL(k_denormalize, gfull, b, 0, p->stream, p->d_full[f], p->n2, field_lb(p, f), field_ub(p, f));
            }
            HIPCHK(hipMemcpyAsync(h, p->d_full[f], (size_t)p->n2 * 4, hipMemcpyDeviceToHost, p->stream));
        }
        HIPCHK(hipStreamSynchronize(p->stream));
        if (touched) p->uploaded = false;   // the caller now holds denormalised fields: a full upload is required before the next sweep
    }
    if (adjoint) {
        if (!p->adj_ready) return fail(SMASHX_E_STATE, "no adjoint sweep has run");
        // parameters_b / states_b are fully overwritten (forward_db.f90:10869-10870); DENORMALIZE_*_B multiplies by (ub-lb)
        for (int f = 0; f < SX_NFIELDS; ++f) {
            float* const hb = host_plane(params_b, states_b, f);
            if (!hb) continue;
            const int s = sx_field_slot(st, f);
            const bool jr = p->opt.njr > 0 && jreg_optim(p, f) > 0;      // inactive cells / unused fields: the regulariser's part
            if (jr) hipLaunchKernelGGL(sx_k_plane_scale, gfull, b, 0, p->stream, p->d_stage, p->d_jg[f], jreg_span(p, f), p->opt.denormalize_forward, p->n2);
            else HIPCHK(hipMemsetAsync(p->d_stage, 0, (size_t)p->n2 * 4, p->stream));
            if (s < 0 && !jr) { std::memset(hb, 0, (size_t)p->n2 * 4); continue; }
            if (s >= 0) hipLaunchKernelGGL(k_scatter, gk, b, 0, p->stream, p->d_stage, slot_vecs(p, s).grad, p->d_cell_flat, p->n, jreg_span(p, f), p->opt.denormalize_forward);
            HIPCHK(hipMemcpyAsync(hb, p->d_stage, (size_t)p->n2 * 4, hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipStreamSynchronize(p->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int smashx_forward(smashx_plan* p, smashx_parameters* params, const smashx_parameters* params_bgd, smashx_states* states,
                   const smashx_states* states_bgd, float* qsim, smashx_costs* costs, smashx_states* fstates) {
    int rc;
    if ((rc = smashx_upload(p, params, params_bgd, states, states_bgd))) return rc;
    if ((rc = smashx_sweep(p, 0, 0.f))) return rc;
    return smashx_download(p, 0, params, states, qsim, costs, fstates, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------------------
// ensemble path: compute_multiple_run (mw_multiple_run.f90:68-119).  Kernels and layout: sx_ensemble.h.
// Samples are processed in batches of SP columns (a multiple of 64) and a batch in time chunks of Tc steps: qt is
// n x Tc x SP x 4 B, both lengths follow from free HBM unless SMASHX_ENS_BATCH / SMASHX_ENS_CHUNK force them.
// Everything of a batch is queued on the plan's stream without a host synchronisation; the batch ends with the copies
// of res_cost / res_qsim.  The plan's own device state (uploaded fields, states, gauge series, timing) is not touched.
// ---------------------------------------------------------------------------------------------------------
namespace {
// the forest (sx_tablehost.h) and what both sample paths hold on the device
int ens_tables(smashx_plan* p) {
    auto& E = p->ens;
    if (E.tables) return 0;
    std::string cycle;
    SxForest F = sx_forest(p->sch, p->h_flwdir_grid.data(), &cycle);
    if (!cycle.empty()) return fail(SMASHX_E_MESH, cycle);
    int rc;
    if ((rc = p->upload_vec(&E.d_up, F.up)) || (rc = p->upload_vec(&E.d_upn, F.upn)) || (rc = p->upload_vec(&E.d_order, F.order))) return rc;
    if ((rc = p->upload_vec(&E.d_gauge_k, p->sch.gauge_k.empty() ? std::vector<int>(1, 0) : p->sch.gauge_k))) return rc;
    if ((rc = p->dmalloc(&E.base, (size_t)SX_NSLOTS * p->npad))) return rc;
    if ((rc = p->dmalloc(&E.plane, (size_t)p->n2))) return rc;
    HIPCHK(hipEventCreate(&E.ev_a)); HIPCHK(hipEventCreate(&E.ev_b));
    E.forest = std::move(F); E.tables = true;
    return 0;
}

// The frame of the two sample paths (smashx_multiple_run, smashx_uniform_costs; host side: sx_samplehost.h).  open: the checks and
// refusals both share, the forest; base: the base fields; arrays: the buffers both need and SxEnsArrays; per batch begin (ev_a, the
// sample up), the path's own launches, costs, end (ev_b, the path's own copies, one synchronisation, the costs into dst).
struct SampleBatches {
    smashx_plan* p = nullptr; std::string who;
    int nfields = 0, nsamples = 0; const float* sample = nullptr;
    int smap[SX_NSLOTS], used_states = 0;          // used_states: bit i = the structure uses state slot i (the ensemble path's init)
    int SP = 0, nbatch = 0, s0 = 0, cnt = 0;       // s0, cnt: first sample and samples of the batch begun
    float* ms = nullptr;                           // device time of the call, summed over the batches
    SxEnsArrays E{}; SxCostArgs C{};
    std::vector<float> hs, hc;

    // reference_call: the reference's routine that never sets denormalize_forward; limit_msg(n): the refusal of more than max_cells
    int open(smashx_plan* plan, const char* name, const char* reference_call, const smashx_parameters* params, const smashx_states* states,
             int nf, const int* ind, const float* smp, int ns, const float* res_cost, long max_cells, std::string (*limit_msg)(int)) {
        p = plan; who = name; nfields = nf; nsamples = ns; sample = smp;
        if (!p || !params || !states || !res_cost) return fail(SMASHX_E_ARG, who + ": null argument (plan, parameters, states, res_cost)");
        if (nsamples < 1) return fail(SMASHX_E_ARG, who + ": nsamples < 1");
        if (nfields < 0 || nfields > SX_NFIELDS || (nfields > 0 && (!ind || !sample))) return fail(SMASHX_E_ARG, who + ": bad nfields / null index list or sample");
        const std::string why = sx_sh_field_map(p->st, nfields, ind, smap);
        if (!why.empty()) return fail(SMASHX_E_ARG, who + ": " + why);
        if (p->opt.denormalize_forward) return fail(SMASHX_E_UNSUPPORTED, who + ": denormalize_forward is not supported (the reference's " + reference_call + " never sets it)");
        if (p->opt.wjreg != 0.f && p->opt.njr > 0) return fail(SMASHX_E_UNSUPPORTED, who + ": wjreg with a regulariser (jreg_fun) is not supported");
        if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, who + ": a tiled plan (tile / owner_mask) is not supported");
        if (wants_signature(p->opt)) return fail(SMASHX_E_UNSUPPORTED, who + ": signature-based jobs_fun are not built into the ensemble cost");
        if (p->n > max_cells) return fail(SMASHX_E_UNSUPPORTED, who + ": " + limit_msg(p->n));
        if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
        const int rc = set_device(p);
        return rc ? rc : ens_tables(p);
    }
    // base fields in cell order; a sampled field needs no base
    int base(const smashx_parameters* params, const smashx_states* states) {
        int rc = close_forcing(p); if (rc) return rc;
        auto& X = p->ens;
        for (int slot = 0; slot < SX_NSLOTS; ++slot) {
            const bool isp = !sx_slot_is_state(slot);
            const int f = sx_slot_field(p->st, slot);
            if (f < 0) continue;
            if (!isp) used_states |= 1 << (slot - SX_NPSLOTS);
            if (smap[slot] >= 0) continue;
            const float* h = host_plane(params, states, f);
            if (!h) return fail(SMASHX_E_ARG, who + ": a " + (isp ? "parameter" : "state") + " field the structure uses is NULL and not sampled");
            HIPCHK(hipMemcpyAsync(X.plane, h, (size_t)p->n2 * 4, hipMemcpyHostToDevice, p->stream));
            hipLaunchKernelGGL(k_gather, dim3((p->n + 255) / 256), dim3(256), 0, p->stream, X.base + (size_t)slot * p->npad, X.plane, p->d_cell_flat, p->n);
        }
        return 0;
    }
    // batches of sp columns, time chunks of tc steps: the buffers both paths need, and what of SxEnsArrays lives in them
    int arrays(int sp, int tc, float* device_ms) {
        auto& X = p->ens;
        const size_t sSP = (size_t)sp, ng1 = (size_t)std::max(p->ng, 1);
        int rc;
        SP = sp; nbatch = (nsamples + SP - 1) / SP; ms = device_ms;
        if ((rc = dev_grow(p, &X.sample, &X.cap_sample, (size_t)std::max(nfields, 1) * sSP)) || (rc = dev_grow(p, &X.qg, &X.cap_qg, ng1 * p->nt * sSP)) ||
            (rc = dev_grow(p, &X.gj, &X.cap_gj, 2 * ng1 * sSP)) || (rc = dev_grow(p, &X.cost, &X.cap_cost, sSP))) return rc;
        E.n = p->n; E.npad = p->npad; E.SP = SP; E.Tc = tc;
        for (int i = 0; i < SX_NSLOTS; ++i) E.smap[i] = smap[i];
        E.base = X.base; E.sample = X.sample; E.up = X.d_up; E.upn = X.d_upn; E.order = X.d_order;
        E.qg = X.qg; E.gauge_k = X.d_gauge_k; E.gj = X.gj; E.med = X.gj + ng1 * sSP; E.cost = X.cost;
        C = cost_args(p, 0.f);
        hs.resize((size_t)std::max(nfields, 1) * sSP); hc.resize(sSP);
        return 0;
    }
    int begin(int bi) {
        if (bi == 0) *ms = 0.f;
        s0 = bi * SP; cnt = std::min(SP, nsamples - s0);
        sx_sh_stage(sample, nfields, nsamples, s0, SP, hs.data());
        HIPCHK(hipEventRecord(p->ens.ev_a, p->stream));
        if (nfields > 0) HIPCHK(hipMemcpyAsync(p->ens.sample, hs.data(), (size_t)nfields * SP * 4, hipMemcpyHostToDevice, p->stream));
        return 0;
    }
    int costs() {          // of qg [g][t][SP]; without a gauge the cost is 0
        if (p->ng == 0) return 0;
        hipLaunchKernelGGL(sx_k_ens_cost_gauge, dim3(SP / 64, p->ng), dim3(64), 0, p->stream, C, E);
        hipLaunchKernelGGL(sx_k_ens_cost_final, dim3(SP / 64), dim3(64), 0, p->stream, C, E);
        HIPCHK(hipMemcpyAsync(hc.data(), p->ens.cost, (size_t)cnt * 4, hipMemcpyDeviceToHost, p->stream));
        return 0;
    }
    int end(float* dst, void* series = nullptr, const void* d_series = nullptr, size_t bytes = 0) {     // series: a copy of the path's own
        HIPCHK(hipEventRecord(p->ens.ev_b, p->stream));
        if (bytes) HIPCHK(hipMemcpyAsync(series, d_series, bytes, hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        HIPCHK(hipGetLastError());
        float t = 0.f;
        if (hipEventElapsedTime(&t, p->ens.ev_a, p->ens.ev_b) == hipSuccess) *ms += t;
        // cost = jobs + wjreg * jreg with jreg = 0 (mwd_cost.f90:300), as smashx_download forms it
        for (int c = 0; c < cnt; ++c) dst[s0 + c] = (p->ng > 0 ? hc[c] : 0.f) + p->opt.wjreg * 0.f;
        return 0;
    }
};
}  // namespace

int smashx_multiple_run(smashx_plan* p, const smashx_parameters* params, const smashx_states* states, int nfields,
                        const int* ind, const float* sample, int nsamples, float* res_cost, float* res_qsim) {
    SampleBatches B;
    int rc = B.open(p, "smashx_multiple_run", "multiple_run", params, states, nfields, ind, sample, nsamples, res_cost, 65535L * SX_ENS_CELLS,
                    [](int) { return std::string("more than 262140 active cells"); });
    if (rc || (rc = B.base(params, states))) return rc;
    auto& X = p->ens;
    hipStream_t sV = p->stream;
    const int st = p->st, n = p->n, nt = p->nt, ng = p->ng;

    // batch size and time chunk
    int SP = 0, Tc = 0;
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    sx_sh_budget(n, nt, ng, nsamples, res_qsim != nullptr, env_int("SMASHX_ENS_BATCH"), env_int("SMASHX_ENS_CHUNK"), (double)fr,
                 4.0 * (double)(X.cap_qt + X.cap_qg + X.cap_qout + X.cap_state), &SP, &Tc);      // what a previous call already holds can be reused
    const int nchunk = (nt + Tc - 1) / Tc;
    const size_t sSP = (size_t)SP;
    if ((rc = B.arrays(SP, Tc, &X.device_ms))) return rc;
    if ((rc = dev_grow(p, &X.state, &X.cap_state, (size_t)SX_NSSLOTS * n * sSP)) || (rc = dev_grow(p, &X.qt, &X.cap_qt, (size_t)n * Tc * sSP))) return rc;
    if (res_qsim && ng > 0 && (rc = dev_grow(p, &X.qout, &X.cap_qout, (size_t)ng * nt * sSP))) return rc;
    SxEnsArrays& E = B.E;
    E.state = X.state; E.qt = X.qt; E.qout = X.qout;
    const dim3 b64(64), bV(64, SX_ENS_CELLS), gV(SP / 64, (n + SX_ENS_CELLS - 1) / SX_ENS_CELLS);
    static void (*const vert[5])(SxDeviceArrays, SxEnsArrays, int, int) = {sx_k_ens_vert_fwd<1>, sx_k_ens_vert_fwd<2>, sx_k_ens_vert_fwd<3>,
                                                                           sx_k_ens_vert_fwd<4>, sx_k_ens_vert_fwd<5>};
    for (int bi = 0; bi < B.nbatch; ++bi) {
        if ((rc = B.begin(bi))) return rc;
        hipLaunchKernelGGL(sx_k_ens_init_states, dim3(SP / 64, std::min(n, 65535)), b64, 0, sV, E, B.used_states);
        for (int c = 0; c < nchunk; ++c) {
            const int t0 = c * Tc, T = std::min(Tc, nt - t0);
            hipLaunchKernelGGL(vert[st - 1], gV, bV, 0, sV, p->A, E, t0, T);
            // one launch per level of the forest: stream order is the dependency
            for (int l = 0; l < X.forest.nlevels; ++l) {
                const int i0 = X.forest.level_begin[l], m = X.forest.level_begin[l + 1] - i0;
                for (int o = 0; o < m; o += 65535)
                    hipLaunchKernelGGL(sx_k_ens_route_fwd, dim3(SP / 64, std::min(65535, m - o)), b64, 0, sV, p->A, E, i0 + o, T);
            }
            if (ng > 0) hipLaunchKernelGGL(sx_k_ens_gauges, dim3(SP / 64, std::min(T, 65535), ng), b64, 0, sV, E, nt, t0, T);
        }
        if ((rc = B.costs())) return rc;
        const bool series = res_qsim && ng > 0;
        if (series) hipLaunchKernelGGL(sx_k_ens_qsim_out, dim3(SP / 64, std::min(nt, 65535)), b64, 0, sV, E, ng, nt);
        if ((rc = B.end(res_cost, series ? res_qsim + (size_t)B.s0 * nt * ng : nullptr, X.qout, series ? (size_t)B.cnt * nt * ng * 4 : 0))) return rc;
    }
    X.info[0] = SP; X.info[1] = Tc; X.info[2] = B.nbatch; X.info[3] = nchunk;
    return 0;
}

int smashx_multiple_run_info(const smashx_plan* p, int info[4], float* device_ms) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (info) for (int i = 0; i < 4; ++i) info[i] = p->ens.info[i];
    if (device_ms) *device_ms = p->ens.device_ms;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// catchment-resident path: smashx_uniform_costs (include/smashx_sbs.h).  Kernel and hand-off: sx_resident.h.  One workgroup per
// sample, so a batch is one launch of SP workgroups followed by the ensemble's two cost kernels on qg [g][t][SP]; the columns past
// the last sample hold whatever the buffer held (nothing of them is copied out).
// ---------------------------------------------------------------------------------------------------------
namespace {
// the per-thread tables of sx_k_res_fwd from the forest of ens_tables; a catchment beyond the kernel's limits is refused once and for all
int res_tables(smashx_plan* p) {
    auto& X = p->ens;
    if (X.res_state) return 0;
    // what a workgroup may claim: the device's limit less what the kernel holds statically (the exact-libm build's tables)
    int lim = 0, dev = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    hipFuncAttributes fa{};
    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&sx_k_res_fwd<1>)));
    X.res_static = fa.sharedSizeBytes;
    const SxResHost R = sx_res_host_tables(X.forest, p->sch.gauge_k, p->ng, (size_t)lim, X.res_static);
    if (!R.refusal.empty()) { X.res_state = 2; X.res_refusal = R.refusal; return 0; }
    int rc;
    if ((rc = p->upload_vec(&X.r_cell, R.cell)) || (rc = p->upload_vec(&X.r_level, R.level)) || (rc = p->upload_vec(&X.r_upline, R.upline)) ||
        (rc = p->upload_vec(&X.r_upn, R.upn)) || (rc = p->upload_vec(&X.r_ownline, R.ownline)) || (rc = p->upload_vec(&X.r_gfirst, R.gfirst)) ||
        (rc = p->upload_vec(&X.r_gnext, R.gnext))) return rc;
    X.res_block = std::max(64, (p->n + 63) / 64 * 64);
    X.res_lds = R.floats * 4;
    X.res_state = 1;
    return 0;
}

}  // namespace

int smashx_uniform_costs(smashx_plan* p, const smashx_parameters* params, const smashx_states* states, int nfields,
                         const int* ind, const float* sample, int nsamples, float* res_cost) {
    SampleBatches B;
    int rc = B.open(p, "smashx_uniform_costs", "optimize_sbs", params, states, nfields, ind, sample, nsamples, res_cost, SX_RES_MAXCELLS, sx_res_cells_refusal);
    if (rc || (rc = res_tables(p))) return rc;
    auto& X = p->ens;
    if (X.res_state == 2) return fail(SMASHX_E_UNSUPPORTED, "smashx_uniform_costs: " + X.res_refusal);
    if ((rc = B.base(params, states))) return rc;
    // samples per batch: one launch of as many workgroups as the batch has samples
    if ((rc = B.arrays(std::min((nsamples + 63) / 64 * 64, 16384), p->nt, &X.res_ms))) return rc;
    SxResTables R{};
    R.nlevels = X.forest.nlevels; R.cell = X.r_cell; R.level = X.r_level; R.upline = X.r_upline; R.upn = X.r_upn; R.ownline = X.r_ownline;
    R.gfirst = X.r_gfirst; R.gnext = X.r_gnext;
    static void (*const kernel[5])(SxDeviceArrays, SxEnsArrays, SxResTables, int) = {sx_k_res_fwd<1>, sx_k_res_fwd<2>, sx_k_res_fwd<3>,
                                                                                       sx_k_res_fwd<4>, sx_k_res_fwd<5>};
    const auto res = kernel[p->st - 1];
    std::vector<float> out(nsamples);
    for (int bi = 0; bi < B.nbatch; ++bi) {
        if ((rc = B.begin(bi))) return rc;
        if (p->ng > 0) {    // without a gauge the cost is 0 and nothing has to run
            if (X.res_lds > 48 * 1024)
                HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(res), hipFuncAttributeMaxDynamicSharedMemorySize, (int)X.res_lds));
            hipLaunchKernelGGL(res, dim3(B.cnt), dim3(X.res_block), X.res_lds, p->stream, p->A, B.E, R, p->nt);
        }
        if ((rc = B.costs()) || (rc = B.end(out.data()))) return rc;
    }
    for (int i = 0; i < nsamples; ++i) res_cost[i] = out[i];      // only a complete call writes res_cost
    X.res_info[0] = p->n; X.res_info[1] = X.forest.nlevels; X.res_info[2] = X.res_block; X.res_info[3] = (int)(X.res_lds + X.res_static);
    return 0;
}

int smashx_uniform_costs_info(const smashx_plan* p, int info[4], float* device_ms) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (info) for (int i = 0; i < 4; ++i) info[i] = p->ens.res_info[i];
    if (device_ms) *device_ms = p->ens.res_ms;
    return 0;
}

// ---- what the two regional maps (smashx_hyper_*, smashx_ann_*) do alike: descriptors, timed upload and gradient, read-back ---------------
namespace {
// the descriptors gathered to plan-cell order and, on first use, the order of the adjoint's sums.  They go up, and *changed is set, only
// when they differ BY BITS from the host copy (a calibration hands the same ones over before every evaluation; NaN == NaN, +0 != -0)
int set_descriptors(smashx_plan* p, smashx_plan::Descriptors& D, int nd, const float* descriptor, bool* changed) {
    int rc;
    std::vector<float> g;
    sx_hh_gather(descriptor, nd, (size_t)p->n2, p->sch.cell_flat, g);
    if (!D.d_order && (rc = p->upload_vec(&D.d_order, sx_hh_order(p->sch.cell_flat)))) return rc;
    *changed = !(D.have && D.nd == nd && g.size() == D.h_desc.size() && (g.empty() || std::memcmp(g.data(), D.h_desc.data(), g.size() * 4) == 0));
    if (*changed) {
        if ((rc = dev_grow(p, &D.d_desc, &D.desc_cap, std::max<size_t>(g.size(), 1)))) return rc;
        if (!g.empty()) HIPCHK(hipMemcpy(D.d_desc, g.data(), g.size() * 4, hipMemcpyHostToDevice));
        D.h_desc.swap(g);
    }
    D.nd = nd; D.have = true;
    return 0;
}
int map_events(smashx_plan::MapTiming& T) { for (hipEvent_t& e : T.ev) if (!e) HIPCHK(hipEventCreate(&e)); return 0; }
// entry e of a launch of the map / terms kernels: field f in its slot's cell vectors and plane
void slot_entry(smashx_plan* p, SxHmFields& F, int e, int f, int slot, bool grad) {
    const SlotVecs V = slot_vecs(p, slot);
    F.val[e] = V.val; F.start[e] = V.start != V.val ? V.start : nullptr; F.full[e] = p->d_full[f];
    F.grad[e] = grad ? V.grad : nullptr;
}
extern "C++" {
// ev[0], the map, ev[1], the routing's preparation on the mapped fields, one synchronisation
template <class Map> int timed_upload(smashx_plan* p, smashx_plan::MapTiming& T, Map&& map) {
    HIPCHK(hipEventRecord(T.ev[0], p->stream));
    map();
    HIPCHK(hipEventRecord(T.ev[1], p->stream));
    hipLaunchKernelGGL(sx_k_prep_routing, dim3((p->n + 255) / 256), dim3(256), 0, p->stream, p->A);
    p->jr_ready = false;
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventElapsedTime(&T.map_ms, T.ev[0], T.ev[1]));
    return 0;
}
// ev[2], the sums zeroed, the path's span loop, ev[3], the sums to the host, one synchronisation
template <class S, class Spans> int timed_gradient(smashx_plan* p, smashx_plan::MapTiming& T, S* d_sums, std::vector<S>& sums, Spans&& spans) {
    HIPCHK(hipEventRecord(T.ev[2], p->stream));
    HIPCHK(hipMemsetAsync(d_sums, 0, sums.size() * sizeof(S), p->stream));
    spans();
    HIPCHK(hipEventRecord(T.ev[3], p->stream));
    HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sums.size() * sizeof(S), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventElapsedTime(&T.grad_ms, T.ev[2], T.ev[3]));
    return 0;
}
}  // extern "C++"
// a cell vector of the device into the active cells of a caller's plane
int read_back(smashx_plan* p, const float* src, std::vector<float>& cellv, float* plane) {
    HIPCHK(hipMemcpyAsync(cellv.data(), src, (size_t)p->n * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    sx_hh_scatter(cellv.data(), p->sch.cell_flat, plane);
    return 0;
}
}  // namespace

// ---- hyper maps on the device (include/smashx_hyper.h, sx_hypermap.h) ------------------------------------------------------------
namespace {
// what every smashx_hyper_* call but set_descriptors refuses, in the order of the header's table
int hyper_refusal(const smashx_plan* p, const char* who) {
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, std::string(who) + ": a tiled plan (an ordered whole-grid sum does not split across parts)");
    if (!p->hyp.dsc.have) return fail(SMASHX_E_STATE, std::string(who) + ": no descriptors set (smashx_hyper_set_descriptors)");
    if (!p->hyp.options) return fail(SMASHX_E_STATE, std::string(who) + ": options not set (the bounds of the maps are those of smashx_set_options)");
    if (p->opt.denormalize_forward) return fail(SMASHX_E_UNSUPPORTED, std::string(who) + ": denormalize_forward (base_hyper_forward does not know it)");
    if (p->opt.njr > 0) return fail(SMASHX_E_UNSUPPORTED, std::string(who) + ": a regulariser (hyper_compute_cost: cost = jobs)");
    return 0;
}
// the fields with a slot, as one launch of the map / terms kernels
SxHmFields hyper_slot_fields(smashx_plan* p, bool grad) {
    SxHmFields F{};
    for (int s = 0; s < SX_NSLOTS; ++s) {
        const int f = sx_slot_field(p->st, s);
        if (f < 0) continue;
        const int e = F.nf++;
        F.field[e] = f; F.lb[e] = field_lb(p, f); F.w[e] = field_ub(p, f) - field_lb(p, f);
        slot_entry(p, F, e, f, s, grad);
    }
    return F;
}
// the fields of F from the hyper matrices and the descriptors the plan holds
void hyper_map(smashx_plan* p, const SxHmFields& F) {
    const smashx_plan::Hyper& H = p->hyp;
    const dim3 b(256), g((p->n + 255) / 256, F.nf);
    if (H.mapping == SMASHX_HYPER_POLYNOMIAL)
        hipLaunchKernelGGL(sx_k_hyper_map<true>, g, b, 0, p->stream, F, H.d_h, H.dsc.d_desc, p->d_cell_flat, H.dsc.nd, H.nh, p->n);
    else
        hipLaunchKernelGGL(sx_k_hyper_map<false>, g, b, 0, p->stream, F, H.d_h, H.dsc.d_desc, p->d_cell_flat, H.dsc.nd, H.nh, p->n);
}
}  // namespace

int smashx_hyper_set_descriptors(smashx_plan* p, int mapping, int nd, const float* descriptor) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    if (const char* why = sx_hh_bad_arguments(mapping, nd)) return fail(SMASHX_E_ARG, why);
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_hyper_set_descriptors: a tiled plan (an ordered whole-grid sum does not split across parts)");
    smashx_plan::Hyper& H = p->hyp;
    if (nd > 0 && !descriptor) { H.dsc.have = H.mapped = false; return 0; }
    int rc = set_device(p); if (rc) return rc;
    bool changed = false;
    if ((rc = set_descriptors(p, H.dsc, nd, descriptor, &changed))) return rc;
    if (changed || H.mapping != mapping) H.mapped = false;
    H.mapping = mapping; H.nh = sx_hh_nhyper(mapping, nd);
    return 0;
}

int smashx_hyper_upload(smashx_plan* p, const float* hyper_parameters, const float* hyper_states) {
    if (!p || !hyper_parameters || !hyper_states) return fail(SMASHX_E_ARG, "null argument");
    int rc = hyper_refusal(p, "smashx_hyper_upload"); if (rc) return rc;
    if ((rc = set_device(p))) return rc;
    smashx_plan::Hyper& H = p->hyp;
    const int nh = H.nh;
    if ((rc = dev_grow(p, &H.d_h, &H.h_cap, (size_t)nh * SX_NFIELDS)) || (rc = map_events(H.tm))) return rc;
    HIPCHK(hipMemcpyAsync(H.d_h, hyper_parameters, (size_t)nh * SMASHX_GNP * 4, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(H.d_h + (size_t)nh * SMASHX_GNP, hyper_states, (size_t)nh * SMASHX_GNS * 4, hipMemcpyHostToDevice, p->stream));
    const SxHmFields F = hyper_slot_fields(p, false);
    if ((rc = timed_upload(p, H.tm, [&] { hyper_map(p, F); }))) return rc;
    p->uploaded = true;
    H.mapped = true;
    return 0;
}

int smashx_hyper_gradient(smashx_plan* p, float* hyper_parameters_b, float* hyper_states_b) {
    if (!p || !hyper_parameters_b || !hyper_states_b) return fail(SMASHX_E_ARG, "null argument");
    int rc = hyper_refusal(p, "smashx_hyper_gradient"); if (rc) return rc;
    smashx_plan::Hyper& H = p->hyp;
    if (!H.mapped || !p->uploaded) return fail(SMASHX_E_STATE, "smashx_hyper_gradient: no smashx_hyper_upload with the descriptors the plan holds");
    if (!(p->adj_ready && p->last_adjoint)) return fail(SMASHX_E_STATE, "smashx_hyper_gradient: the last sweep was not an adjoint sweep");
    if ((rc = set_device(p))) return rc;
    const int nh = H.nh, nd = H.dsc.nd;
    const SxHmFields F = hyper_slot_fields(p, true);
    const int nchain = F.nf * nh;
    // cells per span: from the environment, else what keeps the staging rows at SX_HM_STAGE_BYTES
    int span = env_int("SMASHX_HYPER_SPAN");
    if (span <= 0) span = (int)std::max<size_t>(1024, SX_HM_STAGE_BYTES / ((size_t)nchain * 4));
    span = std::min(span, std::max(p->n, 1));
    if ((rc = dev_grow(p, &H.d_terms, &H.terms_cap, (size_t)span * nchain))) return rc;
    if ((rc = dev_grow(p, &H.d_sums, &H.sums_cap, (size_t)nchain)) || (rc = map_events(H.tm))) return rc;
    H.nchain = nchain; H.span = span;
    std::vector<float> sums((size_t)nchain);
    rc = timed_gradient(p, H.tm, H.d_sums, sums, [&] {
        for (int c0 = 0; c0 < p->n; c0 += span) {
            const int ns = std::min(span, p->n - c0);
            const dim3 b(256), g((ns + 255) / 256, F.nf);
            if (H.mapping == SMASHX_HYPER_POLYNOMIAL)
                hipLaunchKernelGGL(sx_k_hyper_terms<true>, g, b, 0, p->stream, F, H.d_h, H.dsc.d_desc, H.dsc.d_order, nd, nh, p->n, c0, ns, H.d_terms, nchain);
            else
                hipLaunchKernelGGL(sx_k_hyper_terms<false>, g, b, 0, p->stream, F, H.d_h, H.dsc.d_desc, H.dsc.d_order, nd, nh, p->n, c0, ns, H.d_terms, nchain);
            hipLaunchKernelGGL(sx_k_hyper_walk, dim3((nchain + 63) / 64), dim3(64), 0, p->stream, H.d_terms, ns, nchain, H.d_sums, c0 > 0 ? 1 : 0);
        }
    });
    if (rc) return rc;
    sx_hh_close(sums.data(), F.field, F.nf, nh, hyper_parameters_b, hyper_states_b);
    return 0;
}

int smashx_hyper_fields(smashx_plan* p, smashx_parameters* params, smashx_states* states) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    int rc = hyper_refusal(p, "smashx_hyper_fields"); if (rc) return rc;
    smashx_plan::Hyper& H = p->hyp;
    if (!H.mapped) return fail(SMASHX_E_STATE, "smashx_hyper_fields: no smashx_hyper_upload with the descriptors the plan holds");
    if ((rc = set_device(p))) return rc;
    if (!H.d_tmp && (rc = p->dmalloc(&H.d_tmp, (size_t)std::max(p->n, 1)))) return rc;
    std::vector<float> cellv((size_t)p->n);
    for (int f = 0; f < SX_NFIELDS; ++f) {
        float* const h = host_plane(params, states, f);
        if (!h) continue;
        const int s = sx_field_slot(p->st, f);
        const float* src = s >= 0 ? slot_vecs(p, s).start : H.d_tmp;     // what the upload stored; mapped here for a field nothing reads
        if (s < 0) {
            SxHmFields F{};
            F.nf = 1; F.field[0] = f; F.lb[0] = field_lb(p, f); F.w[0] = field_ub(p, f) - field_lb(p, f); F.val[0] = H.d_tmp;
            hyper_map(p, F);
        }
        if ((rc = read_back(p, src, cellv, h))) return rc;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int smashx_hyper_info(const smashx_plan* p, int info[4], float device_ms[2]) {
    if (!p || !info || !device_ms) return fail(SMASHX_E_ARG, "null argument");
    const smashx_plan::Hyper& H = p->hyp;
    info[0] = H.dsc.nd; info[1] = H.nh; info[2] = H.nchain; info[3] = H.span;
    device_ms[0] = H.tm.map_ms; device_ms[1] = H.tm.grad_ms;
    return 0;
}

// ---- the ANN regionalisation on the device (include/smashx_ann.h, sx_annmap.h) and its host twin (sx_annhost.h) ---------------------------
namespace {
// what smashx_ann_upload / _gradient / _fields refuse before they look at their own state, in the order of the header's table
int ann_refusal(const smashx_plan* p, const char* who) {
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, std::string(who) + ": a tiled plan (the weight gradient is a whole-grid sum)");
    const smashx_plan::Ann& A = p->ann;
    if (!A.dsc.have) return fail(SMASHX_E_STATE, std::string(who) + ": no descriptors set (smashx_ann_set_descriptors)");
    if (!A.have_net) return fail(SMASHX_E_STATE, std::string(who) + ": no net set (smashx_ann_set_net)");
    if (A.dsc.nd != A.net.nd) return fail(SMASHX_E_STATE, std::string(who) + ": the net's input width is not the number of descriptors");
    if (!p->uploaded) return fail(SMASHX_E_STATE, std::string(who) + ": no smashx_upload of the background fields");
    // compute_jreg reads the planes smashx_upload placed beside the background, not the mapped ones, and its gradient is added at
    // download, behind the cell gradients the adjoint map reads
    if (p->opt.njr > 0) return fail(SMASHX_E_UNSUPPORTED, std::string(who) + ": a regulariser (njr > 0: the cost's jreg term does not see the mapped fields)");
    return 0;
}
// the control fields as one launch: a field with a slot goes to its cell vectors and plane, any other to a cell vector of its own
SxHmFields ann_fields_of(smashx_plan* p, bool grad) {
    smashx_plan::Ann& A = p->ann;
    SxHmFields F{};
    F.nf = A.net.ncv;
    int extra = 0;
    for (int e = 0; e < F.nf; ++e) {
        const int f = A.field[e], s = sx_field_slot(p->st, f);
        F.field[e] = f;
        if (s >= 0) slot_entry(p, F, e, f, s, grad);
        else F.val[e] = A.d_extra + (size_t)extra++ * std::max(p->n, 1);
    }
    return F;
}
int ann_extra_count(const smashx_plan* p) {
    int extra = 0;
    for (int e = 0; e < p->ann.net.ncv; ++e) if (sx_field_slot(p->st, p->ann.field[e]) < 0) ++extra;
    return extra;
}
// the LDS of a workgroup of the map / terms kernels; above 64 KiB a kernel has to be told
int ann_lds(const smashx_plan* p, size_t* lds) {
    *lds = (size_t)p->ann.net.nslots * SX_ANN_BLOCK * sizeof(double);
    if (*lds > 64 * 1024) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sx_k_ann_map), hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sx_k_ann_terms), hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    }
    return 0;
}
int ann_host_net(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper, SxAnnNet* N) {
    const char* why = "";
    const int rc = sx_annh_build(nd, nlayers, kind, width, ncv, lower, upper, N, &why);
    return rc ? fail(rc, std::string("ann graph: ") + why) : 0;
}
}  // namespace

int smashx_ann_set_descriptors(smashx_plan* p, int nd, const float* descriptor) {
    if (!p || !descriptor) return fail(SMASHX_E_ARG, "smashx_ann_set_descriptors: null argument");
    if (nd < 1) return fail(SMASHX_E_ARG, "smashx_ann_set_descriptors: nd < 1");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_ann_set_descriptors: a tiled plan (the weight gradient is a whole-grid sum)");
    int rc = set_device(p); if (rc) return rc;
    bool changed = false;
    if ((rc = set_descriptors(p, p->ann.dsc, nd, descriptor, &changed))) return rc;
    if (changed) p->ann.mapped = false;
    return 0;
}

int smashx_ann_set_net(smashx_plan* p, int nlayers, const int* kind, const int* width, int ncv, const int* field,
                       const double* lower, const double* upper) {
    if (!p || !kind || !width || !field) return fail(SMASHX_E_ARG, "smashx_ann_set_net: null argument");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_ann_set_net: a tiled plan (the weight gradient is a whole-grid sum)");
    if (ncv < 1) return fail(SMASHX_E_ARG, "smashx_ann_set_net: ncv < 1");
    if (ncv > SX_ANN_MAXCV) return fail(SMASHX_E_UNSUPPORTED, "smashx_ann_set_net: ncv > 24");
    for (int e = 0; e < ncv; ++e) {
        if (field[e] < 0 || field[e] >= SX_NFIELDS) return fail(SMASHX_E_ARG, "smashx_ann_set_net: field outside 0 .. 23");
        for (int q = 0; q < e; ++q) if (field[q] == field[e]) return fail(SMASHX_E_ARG, "smashx_ann_set_net: a field named twice");
    }
    // the net's input width is the number of descriptors the plan holds.  Without descriptors the call is refused with SMASHX_E_STATE; the
    // graph is still built first, with a stand-in width of 1, only so that a graph that is none ranks ahead of that (SMASHX_E_ARG)
    smashx_plan::Ann& A = p->ann;
    SxAnnNet N{};
    int rc = ann_host_net(A.dsc.have ? A.dsc.nd : 1, nlayers, kind, width, ncv, lower, upper, &N); if (rc) return rc;
    if (!A.dsc.have) return fail(SMASHX_E_STATE, "smashx_ann_set_net: no descriptors set (their number is the net's input width)");
    if (const char* why = sx_annh_device_refusal(N)) return fail(SMASHX_E_UNSUPPORTED, std::string("smashx_ann_set_net: ") + why);
    A.net = N;
    for (int e = 0; e < ncv; ++e) A.field[e] = field[e];
    A.have_net = true; A.mapped = false;
    return 0;
}

int smashx_ann_upload(smashx_plan* p, const double* weights) {
    if (!p || !weights) return fail(SMASHX_E_ARG, "smashx_ann_upload: null argument");
    int rc = ann_refusal(p, "smashx_ann_upload"); if (rc) return rc;
    if ((rc = set_device(p))) return rc;
    smashx_plan::Ann& A = p->ann;
    size_t lds = 0;
    if ((rc = dev_grow(p, &A.d_w, &A.w_cap, (size_t)A.net.nw))) return rc;
    if ((rc = dev_grow(p, &A.d_extra, &A.extra_cap, (size_t)std::max(ann_extra_count(p), 1) * std::max(p->n, 1)))) return rc;
    if ((rc = map_events(A.tm)) || (rc = ann_lds(p, &lds))) return rc;
    HIPCHK(hipMemcpyAsync(A.d_w, weights, (size_t)A.net.nw * 8, hipMemcpyHostToDevice, p->stream));
    const SxHmFields F = ann_fields_of(p, false);
    const dim3 b(SX_ANN_BLOCK), g((p->n + SX_ANN_BLOCK - 1) / SX_ANN_BLOCK);
    rc = timed_upload(p, A.tm, [&] {
        if (p->n > 0) hipLaunchKernelGGL(sx_k_ann_map, g, b, lds, p->stream, A.net, F, A.d_w, A.dsc.d_desc, p->d_cell_flat, p->n);
    });
    if (rc) return rc;
    p->last_adjoint = 0;           // a gradient belongs to a sweep behind THIS upload
    A.mapped = true;
    return 0;
}

int smashx_ann_gradient(smashx_plan* p, double* weights_b) {
    if (!p || !weights_b) return fail(SMASHX_E_ARG, "smashx_ann_gradient: null argument");
    int rc = ann_refusal(p, "smashx_ann_gradient"); if (rc) return rc;
    smashx_plan::Ann& A = p->ann;
    if (!A.mapped) return fail(SMASHX_E_STATE, "smashx_ann_gradient: no smashx_ann_upload with the descriptors and the net the plan holds");
    if (!(p->adj_ready && p->last_adjoint)) return fail(SMASHX_E_STATE, "smashx_ann_gradient: no adjoint sweep behind the smashx_ann_upload");
    if ((rc = set_device(p))) return rc;
    const int nw = A.net.nw;
    // cells per span, whole blocks: from the environment, else what keeps the staging rows at SX_ANN_STAGE_BYTES
    long span = env_int("SMASHX_ANN_SPAN");
    if (span <= 0) span = (long)std::max<size_t>(16, SX_ANN_STAGE_BYTES / ((size_t)nw * 8)) * SX_ANN_BLOCK;
    span = (span + SX_ANN_BLOCK - 1) / SX_ANN_BLOCK * SX_ANN_BLOCK;
    span = std::min<long>(span, (std::max(p->n, 1) + SX_ANN_BLOCK - 1) / SX_ANN_BLOCK * SX_ANN_BLOCK);
    size_t lds = 0;
    if ((rc = dev_grow(p, &A.d_terms, &A.terms_cap, (size_t)(span / SX_ANN_BLOCK) * nw))) return rc;
    if ((rc = dev_grow(p, &A.d_sums, &A.sums_cap, (size_t)nw))) return rc;
    if ((rc = map_events(A.tm)) || (rc = ann_lds(p, &lds))) return rc;
    A.span = (int)span;
    const SxHmFields F = ann_fields_of(p, true);
    std::vector<double> sums((size_t)nw);
    rc = timed_gradient(p, A.tm, A.d_sums, sums, [&] {
        for (long c0 = 0; c0 < p->n; c0 += span) {
            const int ns = (int)std::min<long>(span, p->n - c0);
            const int nb = (ns + SX_ANN_BLOCK - 1) / SX_ANN_BLOCK;
            hipLaunchKernelGGL(sx_k_ann_terms, dim3(nb), dim3(SX_ANN_BLOCK), lds, p->stream, A.net, F, A.d_w, A.dsc.d_desc, A.dsc.d_order, p->n, (int)c0, ns, A.d_terms);
            hipLaunchKernelGGL(sx_k_ann_walk, dim3((nw + 63) / 64), dim3(64), 0, p->stream, A.d_terms, nb, nw, A.d_sums);
        }
    });
    if (rc) return rc;
    std::memcpy(weights_b, sums.data(), (size_t)nw * 8);
    return 0;
}

int smashx_ann_fields(smashx_plan* p, smashx_parameters* params, smashx_states* states) {
    if (!p) return fail(SMASHX_E_ARG, "null plan");
    int rc = ann_refusal(p, "smashx_ann_fields"); if (rc) return rc;
    smashx_plan::Ann& A = p->ann;
    if (!A.mapped) return fail(SMASHX_E_STATE, "smashx_ann_fields: no smashx_ann_upload with the descriptors and the net the plan holds");
    if ((rc = set_device(p))) return rc;
    const SxHmFields F = ann_fields_of(p, false);
    std::vector<float> cellv((size_t)p->n);
    for (int e = 0; e < F.nf; ++e) {
        float* const h = host_plane(params, states, F.field[e]);
        if (!h) continue;
        // what the upload stored: a state's starting values
        if ((rc = read_back(p, F.start[e] ? F.start[e] : F.val[e], cellv, h))) return rc;
    }
    return 0;
}

int smashx_ann_info(const smashx_plan* p, int info[4], float device_ms[2]) {
    if (!p || !info || !device_ms) return fail(SMASHX_E_ARG, "null argument");
    const smashx_plan::Ann& A = p->ann;
    info[0] = A.dsc.nd; info[1] = A.have_net ? A.net.nw : 0; info[2] = A.span; info[3] = A.have_net ? A.net.nslots * SX_ANN_BLOCK * 8 : 0;
    device_ms[0] = A.tm.map_ms; device_ms[1] = A.tm.grad_ms;
    return 0;
}

int smashx_ann_host_nweights(int nd, int nlayers, const int* kind, const int* width, int ncv) {
    SxAnnNet N{};
    const std::vector<double> zero((size_t)std::max(ncv, 1), 0.0);
    const int rc = ann_host_net(nd, nlayers, kind, width, ncv, zero.data(), zero.data(), &N);
    return rc ? rc : N.nw;
}
int smashx_ann_host_forward(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper,
                            const double* weights, long n, const float* x, float* y) {
    SxAnnNet N{};
    int rc = ann_host_net(nd, nlayers, kind, width, ncv, lower, upper, &N); if (rc) return rc;
    if (n < 0 || !weights || (n > 0 && (!x || !y))) return fail(SMASHX_E_ARG, "smashx_ann_host_forward: null argument");
    sx_annh_forward(N, weights, (size_t)n, x, (size_t)nd, 1, y);
    return 0;
}
int smashx_ann_host_gradient(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper,
                             const double* weights, long n, const float* x, const float* loss_grad, double* weights_b) {
    SxAnnNet N{};
    int rc = ann_host_net(nd, nlayers, kind, width, ncv, lower, upper, &N); if (rc) return rc;
    if (n < 0 || !weights || !weights_b || (n > 0 && (!x || !loss_grad))) return fail(SMASHX_E_ARG, "smashx_ann_host_gradient: null argument");
    sx_annh_gradient(N, weights, (size_t)n, x, (size_t)nd, 1, loss_grad, weights_b);
    return 0;
}
int smashx_ann_host_activation(int kind, long n, const double* x, double* y, double* dy) {
    if (kind < SMASHX_ANN_RELU || kind > SMASHX_ANN_TANH) return fail(SMASHX_E_ARG, "smashx_ann_host_activation: SMASHX_ANN_RELU .. SMASHX_ANN_TANH expected");
    if (n < 0 || (n > 0 && (!x || !y))) return fail(SMASHX_E_ARG, "smashx_ann_host_activation: null argument");
    const SxAnnNet N{};
    for (long i = 0; i < n; ++i) {
        y[i] = sx_ann_value(N, kind, 0, x[i]);
        if (dy) dy[i] = sx_ann_slope(N, kind, 0, x[i]);
    }
    return 0;
}
int smashx_ann_host_exp(long n, const double* x, double* y) {
    if (n < 0 || (n > 0 && (!x || !y))) return fail(SMASHX_E_ARG, "smashx_ann_host_exp: null argument");
    for (long i = 0; i < n; ++i) y[i] = sx_ann_exp(x[i]);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The set-up products on the resident forcing go in pieces, so that no launch runs for more than a fraction of a second at any grid
// size; SMASHX_*_PIECE in the environment overrides the piece (experiments; tests force several launches with it).
// ---------------------------------------------------------------------------------------------------------
namespace {
// entries per launch: whole blocks of 64, one at least
int piece_entries(const char* env, int preset) {
    const char* e = getenv(env);
    return std::max(64, e ? atoi(e) : preset) / 64 * 64;
}
// ev0, launch(0) .. launch(npieces - 1) with the launch error taken after each, ev1
hipError_t launch_pieces(smashx_plan* p, long npieces, int* launches, const std::function<void(long)>& launch) {
    hipError_t err = hipEventRecord(p->ev0, p->stream);
    for (*launches = 0; *launches < npieces && err == hipSuccess; ++*launches) { launch(*launches); err = hipGetLastError(); }
    return err == hipSuccess ? hipEventRecord(p->ev1, p->stream) : err;
}
// the device time of the SMASHX_VERBOSE lines: from ev0 to ev1
float device_ms(smashx_plan* p) { float ms = 0.f; (void)hipEventElapsedTime(&ms, p->ev0, p->ev1); return ms; }
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// adjust_interception_store (mw_interception_store.f90:19-160) on the resident forcing: kernel and mapping in sx_interception.h.
// One pass over the period per launch; the cells go in pieces of SX_ICI_PIECE (SMASHX_ICI_PIECE).
// ---------------------------------------------------------------------------------------------------------
#define SX_ICI_PIECE (1 << 19)
int smashx_adjust_interception(smashx_plan* p, int nday, const int* day_index, float* ci) {
    if (!p || !day_index || !ci) return fail(SMASHX_E_ARG, "smashx_adjust_interception: null argument (plan, day_index, ci)");
    if (p->st != SMASHX_GR_B && p->st != SMASHX_GR_C)
        return fail(SMASHX_E_UNSUPPORTED, "smashx_adjust_interception: the structure has no interception store (gr-b and gr-c have)");
    const int nt = p->nt;
    if (day_index[0] != 1) return fail(SMASHX_E_ARG, "smashx_adjust_interception: day_index must start at 1");
    for (int t = 1; t < nt; ++t) {
        const int d = day_index[t] - day_index[t - 1];
        if (d != 0 && d != 1) return fail(SMASHX_E_ARG, "smashx_adjust_interception: day_index[" + std::to_string(t) + "] is not the previous day or the one after it");
    }
    if (day_index[nt - 1] != nday) return fail(SMASHX_E_ARG, "smashx_adjust_interception: day_index ends at " + std::to_string(day_index[nt - 1]) + ", nday = " + std::to_string(nday));
    if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
    const int nc = sx_ici_ncand(), rows = (nc + SX_ICI_PER - 1) / SX_ICI_PER;
    if (rows > SX_ICI_ROWS_MAX) return fail(SMASHX_E_UNSUPPORTED, "smashx_adjust_interception: more candidates than the kernel is laid out for");
    if (p->n == 0) return 0;
    int rc = set_device(p); if (rc) return rc;
    if ((rc = close_forcing(p))) return rc;
    int* d_day = nullptr; float* d_ci = nullptr;
    if ((rc = p->dmalloc(&d_day, (size_t)nt))) return rc;
    if ((rc = p->dmalloc(&d_ci, (size_t)p->n))) { p->dfree(d_day); return rc; }
    const int piece = piece_entries("SMASHX_ICI_PIECE", SX_ICI_PIECE);
    std::vector<float> h((size_t)p->n);
    hipStream_t sV = p->stream;
    hipError_t err = hipMemcpyAsync(d_day, day_index, (size_t)nt * sizeof(int), hipMemcpyHostToDevice, sV);
    int launches = 0;
    if (err == hipSuccess) err = launch_pieces(p, ((long)p->n + piece - 1) / piece, &launches, [&](long i) {
        SxDeviceArrays A = p->A;
        A.k0 = (int)(i * piece); A.k1 = (int)std::min((long)p->n, (i + 1) * piece);
        hipLaunchKernelGGL(sx_k_adjust_interception, dim3((A.k1 - A.k0 + 63) / 64), dim3(64, rows), 0, sV, A, d_day, nc, d_ci);
    });
    if (err == hipSuccess) err = hipMemcpyAsync(h.data(), d_ci, (size_t)p->n * sizeof(float), hipMemcpyDeviceToHost, sV);
    if (err == hipSuccess) err = hipStreamSynchronize(sV);
    p->dfree(d_day); p->dfree(d_ci);
    if (err != hipSuccess) return fail(SMASHX_E_HIP, std::string("smashx_adjust_interception: ") + hipGetErrorString(err));
    for (int k = 0; k < p->n; ++k) ci[p->sch.cell_flat[k]] = h[k];       // the plan's own active cells; every other element keeps its value
    if (getenv("SMASHX_VERBOSE"))
        fprintf(stderr, "smashx: adjust_interception %d cells x %d steps x %d candidates: %.3f ms on the device, %d launches\n", p->n, nt, nc, device_ms(p), launches);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// compute_mean_forcing (mw_forcing_statistic.f90:18-75) on the resident forcing: kernel and mapping in sx_meanforcing.h.
// The catchment lists (sx_catchment_lists, sx_tablehost.h: mask_upstream_cells restated, column-major, padded to whole blocks of 64
// entries) are built on the first call and kept with the plan.  A launch covers SX_MF_PIECE entries of every list (SMASHX_MF_PIECE);
// the running sums live in a device buffer of the plan between launches.
// ---------------------------------------------------------------------------------------------------------
#define SX_MF_PIECE (1 << 20)
namespace {
int mf_tables(smashx_plan* p) {
    auto& M = p->mf;
    if (M.state == 1) return 0;
    if (M.state == 2) return fail(SMASHX_E_UNSUPPORTED, M.refusal);
    const int ng = p->ng;
    M.c = sx_catchment_lists(p->sch, p->h_flwdir_grid.data(), ng, &M.refusal);
    if (!M.refusal.empty()) { M.state = 2; return fail(SMASHX_E_UNSUPPORTED, M.refusal); }
    int rc;
    if ((rc = p->upload_vec(&M.d_list, M.c.list))) return rc;
    if ((rc = p->upload_vec(&M.d_begin, M.c.begin))) return rc;
    const size_t ntpad = (size_t)((p->nt + 63) / 64) * 64;
    if ((rc = p->dmalloc(&M.d_state, (size_t)4 * ng * ntpad))) return rc;
    if ((rc = p->dmalloc(&M.d_mp, (size_t)ng * p->nt))) return rc;
    if ((rc = p->dmalloc(&M.d_me, (size_t)ng * p->nt))) return rc;
    M.state = 1;
    return 0;
}
}  // namespace

int smashx_mean_forcing(smashx_plan* p, float* mean_prcp, float* mean_pet) {
    if (!p) return fail(SMASHX_E_ARG, "smashx_mean_forcing: null plan");
    if (!mean_prcp && !mean_pet) return fail(SMASHX_E_ARG, "smashx_mean_forcing: both outputs are null");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_mean_forcing: a tiled plan (tile / owner_mask) is not supported: a sequential sum does not split across parts");
    if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
    if (p->ng == 0) return 0;
    int rc = set_device(p); if (rc) return rc;
    if ((rc = mf_tables(p))) return rc;
    if ((rc = close_forcing(p))) return rc;
    auto& M = p->mf;
    const int ng = p->ng, nt = p->nt;
    const int longest = *std::max_element(M.c.count.begin(), M.c.count.end());
    const int nbp = piece_entries("SMASHX_MF_PIECE", SX_MF_PIECE) / 64;
    hipStream_t sV = p->stream;
    const dim3 grid((unsigned)((nt + 63) / 64), (unsigned)ng), block(64 * SX_LW_WAVES);
    int launches = 0;
    hipError_t err = launch_pieces(p, ((longest + 63) / 64 + nbp - 1) / nbp, &launches, [&](long i) {
#define SX_MF_LAUNCH(C, P, E) hipLaunchKernelGGL((sx_k_mean_forcing<C, P, E>), grid, block, 0, sV, p->A, M.d_list, M.d_begin, ng, (int)(i * nbp), nbp, M.d_state, M.d_mp, M.d_me)
        const bool c = p->A.prcp16 != nullptr;
        if (mean_prcp && mean_pet) { if (c) SX_MF_LAUNCH(true, true, true); else SX_MF_LAUNCH(false, true, true); }
        else if (mean_prcp) { if (c) SX_MF_LAUNCH(true, true, false); else SX_MF_LAUNCH(false, true, false); }
        else { if (c) SX_MF_LAUNCH(true, false, true); else SX_MF_LAUNCH(false, false, true); }
#undef SX_MF_LAUNCH
    });
    const size_t bytes = (size_t)ng * nt * sizeof(float);
    if (err == hipSuccess && mean_prcp) err = hipMemcpyAsync(mean_prcp, M.d_mp, bytes, hipMemcpyDeviceToHost, sV);
    if (err == hipSuccess && mean_pet) err = hipMemcpyAsync(mean_pet, M.d_me, bytes, hipMemcpyDeviceToHost, sV);
    if (err == hipSuccess) err = hipStreamSynchronize(sV);
    if (err != hipSuccess) return fail(SMASHX_E_HIP, std::string("smashx_mean_forcing: ") + hipGetErrorString(err));
    if (getenv("SMASHX_VERBOSE"))
        fprintf(stderr, "smashx: mean_forcing %d gauges x %d steps, longest catchment %d cells, %d list entries: %.3f ms on the device, %d launches\n", ng, nt, longest,
                std::accumulate(M.c.count.begin(), M.c.count.end(), 0), device_ms(p), launches);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// compute_prcp_indices (mw_forcing_statistic.f90:77-220) on the resident rain: kernel and mapping in sx_prcpindices.h.
// The host side (sx_pi_host_tables, sx_tablehost.h) does per gauge what the reference does once per call: the distances, their
// quantiles and bin counts, the catchment and the ten distance bins as one padded list.  The tables are kept with the plan and rebuilt
// when the caller's flwdst differs from the plane they were built for.  A launch covers SX_PI_PIECE list entries of every gauge
// (SMASHX_PI_PIECE).
// ---------------------------------------------------------------------------------------------------------
#define SX_PI_PIECE (1 << 20)
namespace {
void pi_drop(smashx_plan* p) {
    auto& Q = p->pi;
    p->dfree(Q.d_list); p->dfree(Q.d_dl); p->dfree(Q.d_d2l); p->dfree(Q.d_gauges);
    Q.d_list = nullptr; Q.d_dl = Q.d_d2l = nullptr; Q.d_gauges = nullptr;
    Q.state = 0; Q.h_flwdst.clear(); Q.h = SxPiHost();
}

int pi_tables(smashx_plan* p, const float* flwdst) {
    auto& Q = p->pi; const auto& M = p->mf;
    const long n2 = p->n2;
    if (Q.state == 1 && memcmp(Q.h_flwdst.data(), flwdst, (size_t)n2 * sizeof(float)) == 0) return 0;
    pi_drop(p);
    const int ng = p->ng;
    std::string refusal;
    SxPiHost T = sx_pi_host_tables(p->sch, M.c, flwdst, ng, &refusal);
    if (!refusal.empty()) return fail(SMASHX_E_UNSUPPORTED, refusal);
    int rc;
    if ((rc = p->upload_vec(&Q.d_list, T.list)) || (rc = p->upload_vec(&Q.d_dl, T.dl)) || (rc = p->upload_vec(&Q.d_d2l, T.d2l)) ||
        (rc = p->upload_vec(&Q.d_gauges, T.gauges))) return rc;
    if (!Q.d_state) {
        const size_t ntpad = (size_t)((p->nt + 63) / 64) * 64;
        if ((rc = p->dmalloc(&Q.d_state, (size_t)SX_PI_NF * ng * ntpad))) return rc;
        if ((rc = p->dmalloc(&Q.d_out, (size_t)4 * ng * p->nt))) return rc;
        if ((rc = p->dmalloc(&Q.d_flag, (size_t)ng * p->nt))) return rc;
    }
    Q.h_flwdst.assign(flwdst, flwdst + n2);
    T.list = {}; T.dl = {}; T.d2l = {};
    Q.h = std::move(T);
    Q.state = 1;
    return 0;
}
}  // namespace

int smashx_prcp_indices(smashx_plan* p, const float* flwdst, float* prcp_indices) {
    if (!p) return fail(SMASHX_E_ARG, "smashx_prcp_indices: null plan");
    if (!flwdst || !prcp_indices) return fail(SMASHX_E_ARG, "smashx_prcp_indices: null flwdst or prcp_indices");
    if (p->tiled) return fail(SMASHX_E_UNSUPPORTED, "smashx_prcp_indices: a tiled plan (tile / owner_mask) is not supported: a sequential sum does not split across parts");
    if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
    if (p->ng == 0) return 0;
    int rc = set_device(p); if (rc) return rc;
    if ((rc = mf_tables(p))) return rc;
    if ((rc = pi_tables(p, flwdst))) return rc;
    if ((rc = close_forcing(p))) return rc;
    auto& Q = p->pi;
    const int ng = p->ng, nt = p->nt;
    int longest = 0;
    for (int g = 0; g < ng; ++g) longest = std::max(longest, Q.h.gauges[g].sec[SX_PI_NQ]);
    const int nbp = piece_entries("SMASHX_PI_PIECE", SX_PI_PIECE) / 64;
    hipStream_t sV = p->stream;
    const dim3 grid((unsigned)((nt + 63) / 64), (unsigned)ng), block(64 * SX_LW_WAVES);
    int launches = 0;
    hipError_t err = launch_pieces(p, (longest + nbp - 1) / nbp, &launches, [&](long i) {
        const int b0 = (int)(i * nbp);
        if (p->A.prcp16 != nullptr)
            hipLaunchKernelGGL((sx_k_prcp_indices<true>), grid, block, 0, sV, p->A, Q.d_list, Q.d_dl, Q.d_d2l, Q.d_gauges, ng, b0, nbp, Q.d_state, Q.d_out, Q.d_flag);
        else
            hipLaunchKernelGGL((sx_k_prcp_indices<false>), grid, block, 0, sV, p->A, Q.d_list, Q.d_dl, Q.d_d2l, Q.d_gauges, ng, b0, nbp, Q.d_state, Q.d_out, Q.d_flag);
    });
    std::vector<float> h_out((size_t)4 * ng * nt); std::vector<int> h_flag((size_t)ng * nt);
    if (err == hipSuccess) err = hipMemcpyAsync(h_out.data(), Q.d_out, h_out.size() * sizeof(float), hipMemcpyDeviceToHost, sV);
    if (err == hipSuccess) err = hipMemcpyAsync(h_flag.data(), Q.d_flag, h_flag.size() * sizeof(int), hipMemcpyDeviceToHost, sV);
    if (err == hipSuccess) err = hipStreamSynchronize(sV);
    if (err != hipSuccess) return fail(SMASHX_E_HIP, std::string("smashx_prcp_indices: ") + hipGetErrorString(err));
    long written = 0;
    for (size_t o = 0; o < h_flag.size(); ++o) {               // the steps without rain stay as the caller passed them
        if (h_flag[o] != 1) continue;
        memcpy(prcp_indices + o * 4, h_out.data() + o * 4, 4 * sizeof(float));
        ++written;
    }
    if (getenv("SMASHX_VERBOSE"))
        fprintf(stderr, "smashx: prcp_indices %d gauges x %d steps, longest list %d blocks, %ld list entries (%ld of catchments), %ld pairs written: %.3f ms on the device, %d launches\n",
                ng, nt, longest, Q.h.entries, Q.h.catchment_entries, written, device_ms(p), launches);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// tangent model: base_forward_d (forward_db.f90:10517-10601).  One forward sweep that carries the directional
// derivative along (params_d, states_d): vertical kernel on dual numbers, routing twice (values with the hr_imd
// tape, then tangents), cost_d = <d cost / d qsim, qsim_d> + <d(wjreg jreg) / d theta, theta_d> with the adjoint
// seeds of the cost kernels and of the regulariser (fp64 dot products).
// ---------------------------------------------------------------------------------------------------------
int smashx_forward_d(smashx_plan* p, smashx_parameters* params, const smashx_parameters* params_d, const smashx_parameters* params_bgd,
                     smashx_states* states, const smashx_states* states_d, const smashx_states* states_bgd, float* qsim,
                     float* qsim_d, smashx_costs* costs, float* cost_d) {
    if (!p || !params || !states || !params_d || !states_d || !cost_d) return fail(SMASHX_E_ARG, "null argument");
    // a tiled plan: the boundary series of the value pass and then of the tangent pass travel like the forward sweep's (same hooks,
    // same phases), a message per pipeline sub-chunk; the criteria's tangent covers this part's gauges, the regulariser's the whole grid
    // (smashx_tangent_terms gives the two apart: a decomposition adds the parts' first terms and counts the second once)
    if (p->tiled && p->med_nslots > 0) return fail(SMASHX_E_UNSUPPORTED, "tangent model on a tiled plan with the median over gauges of several parts");
    int rc = signature_state(p); if (rc) return rc;
    if ((rc = smashx_upload(p, params, params_bgd, states, states_bgd))) return rc;
    if (!p->have_forcing) return fail(SMASHX_E_STATE, "forcing not set");
    if ((rc = set_device(p))) return rc;
    if ((rc = ensure_chunk_buffers(p, true))) return rc;
    const int st = p->st;
    hipStream_t sV = p->stream, sR = p->stream_r;
    const dim3 b(256), gfull((unsigned)((p->n2 + 255) / 256)), gk((p->n + 255) / 256);
    if (!p->tan_ready) {
        if ((rc = p->dmalloc(&p->A.qtdT, (size_t)p->npad * p->Tc))) return rc;
        if ((rc = p->dmalloc(&p->A.xdT, (size_t)std::max(p->sch.nxslots, 1) * p->Tc))) return rc;
        if ((rc = p->dmalloc(&p->A.qgd, (size_t)std::max(p->ngc, 1) * p->nt))) return rc;
        if ((rc = p->dmalloc(&p->d_qsim_d, (size_t)std::max(p->ng, 1) * p->nt))) return rc;
        HIPCHK(hipMemset(p->A.xdT, 0, (size_t)std::max(p->sch.nxslots, 1) * p->Tc * 4));
        p->tan_ready = true;
    }
    // direction -> per-cell arrays (the gradient arrays double as tangent storage); DENORMALIZE_*_D scales by (ub - lb)
    for (int s = 0; s < SX_NSLOTS; ++s) {
        const int f = sx_slot_field(st, s);
        float* const t = slot_vecs(p, s).grad;
        HIPCHK(hipMemsetAsync(t, 0, (size_t)p->npad * 4, sV));
        if (f < 0) continue;
        const float* h = host_plane(params_d, states_d, f);
        if (!h) return fail(SMASHX_E_ARG, "a tangent field the structure uses is NULL");
        HIPCHK(hipMemcpyAsync(p->d_stage, h, (size_t)p->n2 * 4, hipMemcpyHostToDevice, sV));
        if (p->opt.denormalize_forward)
            hipLaunchKernelGGL(sx_k_plane_scale, gfull, b, 0, sV, p->d_stage, p->d_stage, jreg_span(p, f), 1, p->n2);
        hipLaunchKernelGGL(k_gather, gk, b, 0, sV, t, p->d_stage, p->d_cell_flat, p->n);
        HIPCHK(hipStreamSynchronize(sV));
    }
    // regulariser tangent (COMPUTE_JREG_D, forward_db.f90:2810-2925): the reference's running sums in its order
    float jreg_d = 0.f;
    if (p->opt.njr > 0) {
        HIPCHK(hipEventRecord(p->ev0, sV));
        HIPCHK(hipStreamWaitEvent(p->stream_j, p->ev0, 0));
        if ((rc = run_jreg(p, 0, 0.f))) return rc;                        // jreg itself (cost), fills p->jchains
        HIPCHK(hipStreamSynchronize(p->stream_j));
        float sums_keep[SX_JREG_MAXCHAIN] = {0.f};
        HIPCHK(hipMemcpy(sums_keep, p->d_jsum, sizeof(float) * 2 * p->opt.njr, hipMemcpyDeviceToHost));
        const int nrow = p->cfg.nrow, ncol = p->cfg.ncol;
        // tangent of the control vector as compute_cost sees it: NORMALIZE_D(DENORMALIZE_D(direction))
        for (int idx = 0; idx < SMASHX_GNP + SMASHX_GNS; ++idx) {
            if (jreg_optim(p, idx) <= 0) continue;
            const float* h = host_plane(params_d, states_d, idx);
            if (!h) return fail(SMASHX_E_ARG, "the tangent of an optimised field is NULL");
            if (!p->d_tanplane[idx]) { if ((rc = p->dmalloc(&p->d_tanplane[idx], (size_t)p->n2))) return rc; }
            HIPCHK(hipMemcpyAsync(p->d_tanplane[idx], h, (size_t)p->n2 * 4, hipMemcpyHostToDevice, sV));
            if (p->opt.denormalize_forward) {
                hipLaunchKernelGGL(sx_k_plane_scale, gfull, b, 0, sV, p->d_tanplane[idx], p->d_tanplane[idx], jreg_span(p, idx), 1, p->n2);
                hipLaunchKernelGGL(sx_k_plane_div, gfull, b, 0, sV, p->d_tanplane[idx], jreg_span(p, idx), p->n2);
            }
        }
        const SxJregChains& ch = p->jchains;
        for (int i = 0; i < p->opt.njr; ++i)
            for (int grp = 0; grp < 2; ++grp) {
                const int c = 2 * i + grp, lo = grp ? SMASHX_GNP : 0, hi = grp ? SMASHX_GNP + SMASHX_GNS : SMASHX_GNP;
                long slot = ch.first[c];
                for (int idx = lo; idx < hi; ++idx) {
                    if (jreg_optim(p, idx) <= 0) continue;
                    float* t = p->d_jterm + (size_t)slot++ * p->n2;
                    if (p->opt.jreg_fun[i] == SMASHX_PRIOR)
                        hipLaunchKernelGGL(sx_k_prior_terms_d, gfull, b, 0, sV, t, p->d_jx[idx], p->d_jb[idx], p->d_tanplane[idx], p->n2);
                    else
                        hipLaunchKernelGGL(sx_k_smooth_terms_d, gfull, b, 0, sV, t, p->d_jx[idx], p->d_jb[idx], p->d_tanplane[idx],
                                           p->opt.jreg_fun[i] == SMASHX_SMOOTHING ? 1 : 0, p->d_active, nrow, ncol);
                }
            }
        hipLaunchKernelGGL(sx_k_seq_sum, dim3(ch.nchain), dim3(64), 0, sV, p->d_jterm, ch, p->n2, p->d_jsum);
        float sd[SX_JREG_MAXCHAIN] = {0.f};
        HIPCHK(hipMemcpyAsync(sd, p->d_jsum, sizeof(float) * 2 * p->opt.njr, hipMemcpyDeviceToHost, sV));
        HIPCHK(hipStreamSynchronize(sV));
        HIPCHK(hipMemcpy(p->d_jsum, sums_keep, sizeof(float) * 2 * p->opt.njr, hipMemcpyHostToDevice));   // the download reads jreg from here
        jreg_d = jreg_total(p, sd);
    }
    // sweep
    if ((rc = sweep_begin(p, false))) return rc;
    p->dom_q_active = false;
    const Sweep S = sweep_context(p, false);
    for (int c = 0; c < S.C; ++c) {
        const int t0c = c * p->Tc, Tcur = chunk_len(p, c);
        if (c > 0) { hipEvent_t e = p->event(); HIPCHK(hipEventRecord(e, sR)); HIPCHK(hipStreamWaitEvent(sV, e, 0)); }
        vert_tan(p, 0, t0c, Tcur);
        hipEvent_t e = p->event(); HIPCHK(hipEventRecord(e, sV)); HIPCHK(hipStreamWaitEvent(sR, e, 0));
        // routing: values (forward_d's primal forms, hr_imd tape on), then tangents; one launch per round.  A plan with boundary series
        // (tiles) cuts each pass into the pipeline sub-chunks its message buffers hold: receive + unpack, route, pack + send
        const int Tsub = S.halo ? p->Tp : Tcur;
        for (int pass = 1; pass <= 2; ++pass)
            for (int off = 0; off < Tcur; off += Tsub) {
                const int T = std::min(Tsub, Tcur - off);
                float* xarr = pass == 1 ? p->A.xT : p->A.xdT;
                if ((rc = inlet_series(S, xarr, c, off / Tsub, off, t0c + off, T, false))) return rc;
                route_fwd_rounds(p, off, pass == 1, t0c + off, T, sR, 0, p->sch.nrounds, pass);
                if ((rc = outlet_series(S, xarr, off, t0c + off, T))) return rc;
            }
    }
    // cost (values) and its tangent in the reference's summation order
    if ((rc = run_cost(p, 0, 0.f))) return rc;
    float jobs_d = 0.f;
    if (p->ng > 0) {
        SxCostArgs C = cost_args(p, 0.f);
        hipLaunchKernelGGL(k_gauge_rows, dim3((p->nt + 255) / 256, p->ng), dim3(256), 0, sR, p->d_qsim_d, p->A.qgd, p->d_gauge_gid, p->ng, p->nt);
        hipLaunchKernelGGL(sx_k_cost_tangent, dim3(1), dim3(64), 0, sR, C, p->A.qgd, p->d_cost_out + 1);
        HIPCHK(hipMemcpyAsync(&jobs_d, p->d_cost_out + 1, sizeof(float), hipMemcpyDeviceToHost, sR));
    }
    bool stalled = false;
    if ((rc = sweep_end(p, &stalled))) return rc;
    if (stalled) return fail(SMASHX_E_HIP, "chained routing launch stalled");
    *cost_d = jobs_d + p->opt.wjreg * jreg_d;                        // COMPUTE_COST_D (forward_db.f90:3248)
    p->last_jobs_d = jobs_d; p->last_jreg_d = jreg_d;
    if (qsim_d && p->ng > 0) {
        std::vector<float> qd((size_t)p->ng * p->nt);
        HIPCHK(hipMemcpy(qd.data(), p->d_qsim_d, qd.size() * 4, hipMemcpyDeviceToHost));
        for (int g = 0; g < p->ng; ++g)
            for (int t = 0; t < p->nt; ++t) qsim_d[g + (size_t)p->ng * t] = qd[(size_t)g * p->nt + t];
    }
    p->last_adjoint = 0;
    // primal outputs exactly like base_forward (parameters / states denormalised + round trip, states restored)
    return smashx_download(p, 0, params, states, qsim, costs, nullptr, nullptr, nullptr);
}

int smashx_tangent_terms(const smashx_plan* p, float* jobs_d, float* jreg_d) {
    if (!p || !jobs_d || !jreg_d) return fail(SMASHX_E_ARG, "null argument");
    *jobs_d = p->last_jobs_d; *jreg_d = p->last_jreg_d;
    return 0;
}

int smashx_forward_b(smashx_plan* p, smashx_parameters* params, const smashx_parameters* params_bgd, smashx_states* states,
                     const smashx_states* states_bgd, float cost_b, float* qsim, smashx_costs* costs,
                     smashx_parameters* params_b, smashx_states* states_b) {
    int rc;
    if ((rc = smashx_upload(p, params, params_bgd, states, states_bgd))) return rc;
    if ((rc = smashx_sweep(p, 1, cost_b))) return rc;
    return smashx_download(p, 1, params, states, qsim, costs, nullptr, params_b, states_b);
}

}  // extern "C"
