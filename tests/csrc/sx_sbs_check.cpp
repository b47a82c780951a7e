// Stand-alone driver of the step-by-step optimiser (smash_amd/csrc/sx_sbs.cpp) for the sanitizer builds of tests/test_sbs_sanitized.py:
// a closed-form cost -- a weighted squared distance in the transformed space, to a target that lies outside the box for some
// components, so that the run clips, stays on bounds, halves and doubles its step and takes line-search steps -- through the C entry
// points of include/smashx_sbs.h, with the invariants checked on the way (candidates inside the box, batches of 1 .. 2 n, a cost that
// never rises, nfg = 1 + what was asked).  usage: sx_sbs_check n seed maxiter
#include "../../include/smashx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static unsigned long long rng_state;
static double rnd() {
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 3;
    rng_state = argc > 2 ? (unsigned long long)atoll(argv[2]) : 1ULL;
    const int maxiter = argc > 3 ? atoi(argv[3]) : 30;
    std::vector<float> lo(n), up(n), x0(n), target(n), w(n);
    for (int i = 0; i < n; ++i) {
        switch (i % 3) {        // the three transformations: asinh, logit, log
            case 0: lo[i] = -5.f - (float)(10.0 * rnd()); up[i] = 1.f + (float)(5.0 * rnd()); break;
            case 1: lo[i] = 1e-4f; up[i] = 0.5f + (float)(0.49 * rnd()); break;
            default: lo[i] = 1.f + (float)rnd(); up[i] = 100.f + (float)(400.0 * rnd()); break;
        }
        x0[i] = lo[i] + (up[i] - lo[i]) * (float)(0.2 + 0.6 * rnd());
        // every other target lies outside the box
        const double t = rnd();
        target[i] = (i % 2) ? lo[i] + (up[i] - lo[i]) * (float)t : (t < 0.5 ? lo[i] - 0.3f * (up[i] - lo[i]) : up[i] + 0.3f * (up[i] - lo[i]));
        w[i] = 1.f + (float)(3.0 * rnd());
    }
    auto cost = [&](const float* x) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) { const float d = (x[i] - target[i]) / (up[i] - lo[i]); s += w[i] * d * d; }
        return s;
    };
    int bad = 0;
    auto violation = [&](const std::string& what) { printf("VIOLATION %s\n", what.c_str()); ++bad; };

    smashx_sbs* o = nullptr;
    if (smashx_sbs_create(n, lo.data(), up.data(), x0.data(), cost(x0.data()), maxiter, &o) != SMASHX_OK) { printf("VIOLATION create\n"); return 1; }
    std::vector<float> y((size_t)n * 2 * n), f(2 * (size_t)n), x(n);
    float prev = smashx_sbs_gx(o);
    long asked = 0;
    int m = 0, batches = 0, singles = 0;
    for (;;) {
        if (smashx_sbs_ask(o, y.data(), &m) != SMASHX_OK) { violation("ask"); break; }
        if (m == 0) break;
        if (m < 1 || m > 2 * n) { violation("batch size " + std::to_string(m)); break; }
        if (smashx_sbs_ask(o, y.data(), &m) != SMASHX_E_STATE) violation("a second ask with a batch open");
        ++batches; singles += (m == 1);
        for (int c = 0; c < m; ++c) {
            for (int i = 0; i < n; ++i) {
                const float v = y[(size_t)c * n + i], slack = 1e-4f * (fabsf(lo[i]) + fabsf(up[i]));
                if (!(v >= lo[i] - slack && v <= up[i] + slack)) violation("candidate outside the box");
            }
            f[c] = cost(&y[(size_t)c * n]);
        }
        asked += m;
        if (smashx_sbs_tell(o, f.data()) != SMASHX_OK) { violation("tell"); break; }
        const float gx = smashx_sbs_gx(o);
        if (!(gx <= prev)) violation("the cost rose");
        prev = gx;
        if (smashx_sbs_nfg(o) != 1 + asked) violation("nfg");
    }
    if (smashx_sbs_tell(o, f.data()) != SMASHX_E_STATE) violation("tell after the end");
    smashx_sbs_x(o, x.data());
    if (maxiter > 0 && !(fabsf(cost(x.data()) - smashx_sbs_gx(o)) <= 1e-5f * (1.f + fabsf(smashx_sbs_gx(o))))) violation("gx is not the cost at x");
    const std::string msg = smashx_sbs_message(o);
    if (maxiter > 0 && msg.empty()) violation("no message");
    if (smashx_sbs_iter(o) > maxiter * n) violation("more iterations than maxiter * n");
    printf("%s n %d it %d nfg %d batches %d line-search %d ddx %g gx %g %s\n", bad ? "bad" : "ok", n, smashx_sbs_iter(o), smashx_sbs_nfg(o), batches,
           singles, (double)smashx_sbs_ddx(o), (double)smashx_sbs_gx(o), msg.c_str());
    smashx_sbs_destroy(o);
    return bad ? 1 : 0;
}
