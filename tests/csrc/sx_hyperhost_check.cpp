// sx_hyperhost_check.cpp -- the plain-C++ host side of the hyper maps on the device (smash_amd/csrc/sx_hyperhost.h) on a masked grid,
// every buffer a heap block of exactly the size the library's caller owes: built with -fsanitize=address,undefined by
// tests/test_hyper_host_sanitized.py.  argv: nrow ncol nd.  Prints "ok <active cells>" or "VIOLATION ...".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../smash_amd/csrc/sx_hyperhost.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int nrow = atoi(argv[1]), ncol = atoi(argv[2]), nd = atoi(argv[3]);
    const size_t n2 = (size_t)nrow * ncol;
    // argument checks
    if (sx_hh_bad_arguments(SMASHX_HYPER_LINEAR, 0) || sx_hh_bad_arguments(SMASHX_HYPER_POLYNOMIAL, nd)) { puts("VIOLATION good arguments refused"); return 1; }
    if (!sx_hh_bad_arguments(0, nd) || !sx_hh_bad_arguments(3, nd) || !sx_hh_bad_arguments(SMASHX_HYPER_LINEAR, -1)) { puts("VIOLATION bad arguments pass"); return 1; }
    if (sx_hh_nhyper(SMASHX_HYPER_LINEAR, nd) != 1 + nd || sx_hh_nhyper(SMASHX_HYPER_POLYNOMIAL, nd) != 1 + 2 * nd) { puts("VIOLATION nhyper"); return 1; }
    // a ragged mask, the plan's cells in an order of its own (reversed stripes)
    std::vector<int> cell_flat;
    for (int c = ncol - 1; c >= 0; --c)
        for (int r = 0; r < nrow; ++r)
            if ((r * 7 + c * 3) % 5 != 0) cell_flat.push_back(r + c * nrow);
    const size_t n = cell_flat.size();
    std::unique_ptr<float[]> desc(new float[(size_t)nd * n2 + (nd == 0)]);
    for (size_t i = 0; i < (size_t)nd * n2; ++i) desc[i] = (float)i;
    std::vector<float> g;
    sx_hh_gather(nd > 0 ? desc.get() : nullptr, nd, n2, cell_flat, g);
    if (g.size() != (size_t)nd * n) { puts("VIOLATION gather size"); return 1; }
    for (int j = 0; j < nd; ++j)
        for (size_t k = 0; k < n; ++k)
            if (g[(size_t)j * n + k] != (float)((size_t)j * n2 + cell_flat[k])) { puts("VIOLATION gather value"); return 1; }
    const std::vector<int> order = sx_hh_order(cell_flat);
    if (order.size() != n) { puts("VIOLATION order size"); return 1; }
    for (size_t i = 1; i < n; ++i)
        if (!(cell_flat[order[i - 1]] < cell_flat[order[i]])) { puts("VIOLATION order"); return 1; }
    // closing: every structure's fields, both mappings
    for (int st = 1; st <= 5; ++st)
        for (int mapping = SMASHX_HYPER_LINEAR; mapping <= SMASHX_HYPER_POLYNOMIAL; ++mapping) {
            const int nh = sx_hh_nhyper(mapping, nd);
            int field[SX_NFIELDS], nf = 0;
            for (int s = 0; s < SX_NSLOTS; ++s) if (sx_slot_field(st, s) >= 0) field[nf++] = sx_slot_field(st, s);
            std::unique_ptr<float[]> sums(new float[(size_t)nf * nh]), hp(new float[(size_t)nh * SMASHX_GNP]), hs(new float[(size_t)nh * SMASHX_GNS]);
            for (int i = 0; i < nf * nh; ++i) sums[i] = 1.f + (float)i;
            for (int i = 0; i < nh * SMASHX_GNP; ++i) hp[i] = -1.f;
            for (int i = 0; i < nh * SMASHX_GNS; ++i) hs[i] = -1.f;
            sx_hh_close(sums.get(), field, nf, nh, hp.get(), hs.get());
            double total = 0, want = 0;
            for (int i = 0; i < nh * SMASHX_GNP; ++i) { if (hp[i] < 0.f) { puts("VIOLATION close left an entry"); return 1; } total += hp[i]; }
            for (int i = 0; i < nh * SMASHX_GNS; ++i) { if (hs[i] < 0.f) { puts("VIOLATION close left an entry"); return 1; } total += hs[i]; }
            for (int i = 0; i < nf * nh; ++i) want += sums[i];
            if (total != want) { puts("VIOLATION close sum"); return 1; }
        }
    // scatter
    std::unique_ptr<float[]> plane(new float[n2]), cellv(new float[n + (n == 0)]);
    for (size_t i = 0; i < n2; ++i) plane[i] = -7.f;
    for (size_t k = 0; k < n; ++k) cellv[k] = (float)k;
    sx_hh_scatter(cellv.get(), cell_flat, plane.get());
    size_t kept = 0;
    for (size_t i = 0; i < n2; ++i) kept += plane[i] == -7.f;
    if (kept != n2 - n) { puts("VIOLATION scatter"); return 1; }
    for (size_t k = 0; k < n; ++k) if (plane[cell_flat[k]] != (float)k) { puts("VIOLATION scatter value"); return 1; }
    printf("ok %zu\n", n);
    return 0;
}
