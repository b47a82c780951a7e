// sx_sbs.cpp -- the step-by-step optimiser of the uniform calibration: mw_optimize::optimize_sbs (mw_optimize.f90:53-294) restated
// statement by statement and turned inside out (ask / tell, include/smashx_sbs.h).  Host C++, no GPU, no third-party library.
//
// Everything is fp32 with glibc's logf / expf / asinhf / sinhf / powf, and the file is compiled with -ffp-contract=off like the parity
// build of the reference: (1 - clg) * jfa * ddx + clg * sdx(ia) must stay two roundings.  What the reference does between the
// evaluations of one stage depends on x_t, ddx, iaa and jfaa only -- none of them moves before the stage's last cost is in -- so the
// candidates of a stage are formed at once (ask) and their costs are folded in the reference's (i, j) order with its strict `<` (tell).
#include "../../include/smashx.h"

#include <cmath>
#include <string>
#include <vector>

struct smashx_sbs {
    int n = 0, maxiter = 0;
    std::vector<float> x, l, u, x_t, l_t, u_t, z_t, sdx;
    float gx = 0.f, ga = 0.f, clg = 0.f, ddx = 0.f, dxn = 0.f;
    int iter = 0, nfg = 0, ia = 0, iaa = 0, iam = 0, jfaa = 0;
    // the reference reads jfa uninitialised (jfaa = jfa) when the first iteration finds no better point; harmless there because
    // iaa = 0 matches no i.  Here it starts at 0, which no jf = -1 / +1 equals either.
    int jfa = 0;
    enum Stage { COORD, LINE, DONE } stage = COORD;
    bool open = false;                      // a batch has been asked and not told yet
    std::vector<int> ci, cjf;               // the batch: component (1-based) and direction of every candidate
    std::vector<float> cy;                  // ... and its transformed value y_t(i); for LINE the whole y_t
    std::string msg;
};

namespace {
// transformation_sbs / inv_transformation_sbs (mw_optimize.f90:422-481), one component
inline float sbs_fwd(float x, float l, float u) {
    if (l < 0.f) return asinhf(x);
    if (l >= 0.f && u <= 1.f) return logf(x / (1.f - x));
    return logf(x);
}
inline float sbs_inv(float xt, float l, float u) {
    if (l < 0.f) return sinhf(xt);
    if (l >= 0.f && u <= 1.f) return expf(xt) / (1.f + expf(xt));
    return expf(xt);
}
inline void sbs_inv_all(const smashx_sbs* o, const float* t, float* out) {
    for (int i = 0; i < o->n; ++i) out[i] = sbs_inv(t[i], o->l[i], o->u[i]);
}

// the tail of an iteration: mw_optimize.f90:239-290
void sbs_close_iteration(smashx_sbs* o) {
    o->ia = 0;
    o->iter += 1;
    if (o->ddx < 0.01f) { o->stage = smashx_sbs::DONE; o->msg = "CONVERGENCE: DDX < 0.01"; return; }
    if (o->iter == o->maxiter * o->n) { o->stage = smashx_sbs::DONE; o->msg = "STOP: TOTAL NO. OF ITERATION EXCEEDS LIMIT"; return; }
    o->stage = smashx_sbs::COORD;
}

// what follows the coordinate loop: mw_optimize.f90:162-237.  Returns true when a line-search candidate is to be evaluated.
bool sbs_after_coord(smashx_sbs* o) {
    const int n = o->n;
    o->iaa = o->ia;
    o->jfaa = o->jfa;
    if (o->ia != 0) {
        o->x_t = o->z_t;
        sbs_inv_all(o, o->x_t.data(), o->x.data());
        for (int i = 0; i < n; ++i) o->sdx[i] = o->clg * o->sdx[i];
        o->sdx[o->ia - 1] = (1.f - o->clg) * (float)o->jfa * o->ddx + o->clg * o->sdx[o->ia - 1];
        o->iam = o->iam + 1;
        if (o->iam > 2 * n) { o->ddx = o->ddx * 2.f; o->iam = 0; }
        if (o->gx < o->ga - 2.f) o->ga = o->gx;
    } else {
        o->ddx = o->ddx / 2.f;
        o->iam = 0;
    }
    if (o->iter + 1 > 4 * n) {          // the reference's iter is this loop's count + 1 while the iteration runs
        o->cy.assign(n, 0.f);
        for (int i = 0; i < n; ++i) {
            float y = o->x_t[i] + o->sdx[i];
            if (y < o->l_t[i]) y = o->l_t[i];
            if (y > o->u_t[i]) y = o->u_t[i];
            o->cy[i] = y;
        }
        return true;
    }
    return false;
}
}  // namespace

extern "C" {

int smashx_sbs_create(int n, const float* lower, const float* upper, const float* x0, float cost0, int maxiter, smashx_sbs** out) {
    if (!out || !lower || !upper || !x0 || n < 1 || maxiter < 0) return SMASHX_E_ARG;
    if ((long long)maxiter * n > 2147483647LL) return SMASHX_E_ARG;
    for (int i = 0; i < n; ++i) if (lower[i] > upper[i]) return SMASHX_E_ARG;
    smashx_sbs* o = new smashx_sbs();
    o->n = n; o->maxiter = maxiter;
    o->x.assign(x0, x0 + n); o->l.assign(lower, lower + n); o->u.assign(upper, upper + n);
    o->x_t.resize(n); o->l_t.resize(n); o->u_t.resize(n);
    for (int i = 0; i < n; ++i) {
        o->x_t[i] = sbs_fwd(o->x[i], o->l[i], o->u[i]);
        o->l_t[i] = sbs_fwd(o->l[i], o->l[i], o->u[i]);
        o->u_t[i] = sbs_fwd(o->u[i], o->l[i], o->u[i]);
    }
    o->gx = cost0; o->ga = o->gx;
    o->clg = powf(0.7f, 1.f / (float)n);
    o->z_t = o->x_t;
    o->sdx.assign(n, 0.f);
    o->ddx = 0.64f; o->dxn = o->ddx;
    o->nfg = 1;
    if (maxiter * n == 0) o->stage = smashx_sbs::DONE;       // do iter = 1, 0: the loop never runs, no message
    *out = o;
    return 0;
}

int smashx_sbs_destroy(smashx_sbs* o) { delete o; return 0; }

int smashx_sbs_ask(smashx_sbs* o, float* y, int* m) {
    if (!o || !y || !m) return SMASHX_E_ARG;
    if (o->open) return SMASHX_E_STATE;
    const int n = o->n;
    *m = 0;
    for (;;) {
        if (o->stage == smashx_sbs::DONE) return 0;
        if (o->stage == smashx_sbs::LINE) {          // the candidate sbs_after_coord left in cy
            sbs_inv_all(o, o->cy.data(), y);
            *m = 1; o->open = true;
            return 0;
        }
        // head of an iteration: mw_optimize.f90:121-137
        if (o->dxn > o->ddx) o->dxn = o->ddx;
        if (o->ddx > 2.f) o->ddx = o->dxn;
        o->ci.clear(); o->cjf.clear(); o->cy.clear();
        for (int i = 1; i <= n; ++i) {
            const float xt = o->x_t[i - 1], lt = o->l_t[i - 1], ut = o->u_t[i - 1];
            for (int j = 1; j <= 2; ++j) {
                const int jf = 2 * j - 3;
                if (i == o->iaa && jf == -o->jfaa) continue;
                if (xt <= lt && jf < 0) continue;
                if (xt >= ut && jf > 0) continue;
                float yt = xt + (float)jf * o->ddx;
                if (yt < lt) yt = lt;
                if (yt > ut) yt = ut;
                o->ci.push_back(i); o->cjf.push_back(jf); o->cy.push_back(yt);
            }
        }
        const int mm = (int)o->ci.size();
        if (mm > 0) {
            // y_t = x_t with component i replaced; the inverse transformation runs over the whole vector, as the reference's does
            std::vector<float> yt(n);
            for (int c = 0; c < mm; ++c) {
                yt = o->x_t;
                yt[o->ci[c] - 1] = o->cy[c];
                sbs_inv_all(o, yt.data(), y + (size_t)c * n);
            }
            *m = mm; o->open = true;
            return 0;
        }
        // every candidate skipped: the iteration goes on without an evaluation
        if (sbs_after_coord(o)) { o->stage = smashx_sbs::LINE; continue; }
        sbs_close_iteration(o);
    }
}

int smashx_sbs_tell(smashx_sbs* o, const float* cost) {
    if (!o || !cost) return SMASHX_E_ARG;
    if (!o->open) return SMASHX_E_STATE;
    o->open = false;
    if (o->stage == smashx_sbs::COORD) {
        for (size_t c = 0; c < o->ci.size(); ++c) {          // mw_optimize.f90:146-156, in (i, j) order
            const float f = cost[c];
            o->nfg = o->nfg + 1;
            if (f < o->gx) {
                o->z_t = o->x_t;
                o->z_t[o->ci[c] - 1] = o->cy[c];
                o->gx = f;
                o->ia = o->ci[c];
                o->jfa = o->cjf[c];
            }
        }
        if (sbs_after_coord(o)) { o->stage = smashx_sbs::LINE; return 0; }
        sbs_close_iteration(o);
        return 0;
    }
    // the line-search candidate: mw_optimize.f90:215-235
    const float f = cost[0];
    o->nfg = o->nfg + 1;
    if (f < o->gx) {
        o->gx = f;
        o->jfaa = 0;
        o->x_t = o->cy;
        sbs_inv_all(o, o->x_t.data(), o->x.data());
        if (o->gx < o->ga - 2.f) o->ga = o->gx;
    }
    sbs_close_iteration(o);
    return 0;
}

int smashx_sbs_x(const smashx_sbs* o, float* x) {
    if (!o || !x) return SMASHX_E_ARG;
    for (int i = 0; i < o->n; ++i) x[i] = o->x[i];
    return 0;
}
float smashx_sbs_gx(const smashx_sbs* o) { return o ? o->gx : 0.f; }
float smashx_sbs_ddx(const smashx_sbs* o) { return o ? o->ddx : 0.f; }
int smashx_sbs_iter(const smashx_sbs* o) { return o ? o->iter : 0; }
int smashx_sbs_nfg(const smashx_sbs* o) { return o ? o->nfg : 0; }
const char* smashx_sbs_message(const smashx_sbs* o) { return o ? o->msg.c_str() : ""; }

}  // extern "C"
