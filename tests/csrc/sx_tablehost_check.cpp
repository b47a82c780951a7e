/* Host check of the table builders of the sample paths and the forcing statistics (smash_amd/csrc/sx_tablehost.h), built with
 * -fsanitize=address,undefined -ffp-contract=off by tests/test_table_host_sanitized.py.  Reads a mesh from stdin (nrow ncol, then flwdir
 * and active_cell, column-major, then ng and the gauge rows and columns; optionally "flwdst" and the plane as fp32 bit patterns,
 * optionally "lds" and the bytes a workgroup may claim and the kernel holds statically), builds the schedule (sx_plan.cpp) for
 * cell_flat, k_of_flat and gauge_k, runs the four builders with every input in a heap block of exactly its size, verifies their
 * invariants (VIOLATION ... on failure) and prints every table as "name v v v ..." (floats as bit patterns), a refusal as
 * "name_refusal text", then "ok".  A mesh the schedule builder refuses for a cycle is given plain column-major numbering, so that
 * the forest's own refusal is reached. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../smash_amd/csrc/sx_tablehost.h"

#define REQUIRE(c, msg) do { if (!(c)) { std::printf("VIOLATION %s (line %d)\n", msg, __LINE__); return 2; } } while (0)

static void put(const char* name, const std::vector<int>& v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static void put(const char* name, const std::vector<float>& v) {
    std::printf("%s", name);
    for (float x : v) std::printf(" %u", bits(x));
    std::printf("\n");
}

static int check_forest(const SxSchedule& s, const signed char* fd, const SxForest& F) {
    const int n = s.n;
    REQUIRE(F.n == n && (int)F.order.size() == n && (int)F.level_begin.size() == F.nlevels + 1, "forest sizes");
    std::vector<int> seen(n, 0);
    REQUIRE(F.level_begin[0] == 0 && F.level_begin[F.nlevels] == n, "levels cover the cells");
    for (int l = 0; l < F.nlevels; ++l)
        for (int i = F.level_begin[l]; i < F.level_begin[l + 1]; ++i) {
            const int k = F.order[i];
            REQUIRE(k >= 0 && k < n, "order entry");
            REQUIRE(F.level[k] == l, "a cell sits in the level it is listed under");
            REQUIRE(i == F.level_begin[l] || F.order[i - 1] < k, "ascending plan index inside a level");
            seen[k]++;
        }
    for (int k = 0; k < n; ++k) REQUIRE(seen[k] == 1, "every cell in exactly one level");
    long links = 0, roots = 0;
    for (int k = 0; k < n; ++k) {
        REQUIRE(F.upn[k] >= 0 && F.upn[k] <= 8, "upstream count");
        int want = 0;
        for (int c = 0; c < 8; ++c) {
            const int u = F.up[(size_t)k * 8 + c];
            if (c >= F.upn[k]) { REQUIRE(u == -1, "unused upstream entry"); continue; }
            REQUIRE(u >= 0 && u < n, "upstream entry");
            REQUIRE(F.level[u] < F.level[k], "an upstream cell lies in a strictly lower level");
            REQUIRE(F.parent[u] == k, "parent and up agree");
            REQUIRE(c == 0 || fd[s.cell_flat[F.up[(size_t)k * 8 + c - 1]]] < fd[s.cell_flat[u]], "upstream cells in strictly ascending D8 code");
            want = std::max(want, F.level[u] + 1);
            ++links;
        }
        REQUIRE(F.level[k] == want, "level is the longest path from the leaves");
        if (F.parent[k] < 0) ++roots;
        else REQUIRE(F.parent[k] < n, "parent entry");
    }
    REQUIRE(links + roots == n, "every cell but the roots is listed upstream of its parent");
    return 0;
}

static int check_res(const SxForest& F, const std::vector<int>& gauge_k, int ng, const SxResHost& R) {
    const int n = F.n;
    std::vector<int> pos(n);
    for (int i = 0; i < n; ++i) pos[F.order[i]] = i;
    std::vector<char> taken(R.floats, 0);
    for (int i = 0; i < n; ++i) {
        const int k = R.cell[i], own = R.ownline[i];
        REQUIRE(k == F.order[i] && R.level[i] == F.level[k] && R.upn[i] == F.upn[k], "thread i holds cell order[i]");
        REQUIRE((own == -1) == (F.parent[k] < 0), "no line exactly for the roots");
        if (own != -1) {
            const int lg = own & 31, D = F.level[F.parent[k]] - F.level[k];
            const size_t first = (size_t)(own >> 5), slots = (size_t)1 << lg;
            REQUIRE(own >= 0 && lg >= 1 && first + slots <= R.floats, "line inside the floats");
            REQUIRE((1 << lg) >= D + 1 && ((1 << (lg - 1)) < D + 1 || lg == 1), "D + 1 slots rounded up to a power of two");
            for (size_t j = first; j < first + slots; ++j) { REQUIRE(!taken[j], "lines are disjoint"); taken[j] = 1; }
        }
        for (int c = 0; c < R.upn[i]; ++c)
            REQUIRE(R.upline[(size_t)i * 8 + c] == R.ownline[pos[F.up[(size_t)k * 8 + c]]], "upline is the own line of that child");
    }
    std::vector<int> met(std::max(ng, 1), 0);
    for (int i = 0; i < n; ++i) {
        int last = -1;
        for (int g = R.gfirst[i]; g != -1; g = R.gnext[g]) {
            REQUIRE(g > last && g < ng, "chain in ascending gauge order");
            REQUIRE(gauge_k[g] == R.cell[i], "a chain holds the gauges of its cell");
            met[g]++; last = g;
        }
    }
    for (int g = 0; g < ng; ++g) REQUIRE(met[g] == (gauge_k[g] >= 0 && gauge_k[g] < n ? 1 : 0), "every gauge in exactly one chain");
    return 0;
}

// entries [b0, b1) of list: `real` plan cells, then -1 up to a whole number of blocks of 64
static int check_section(const std::vector<int>& list, long b0, long b1, long real, int n) {
    REQUIRE(b0 % 64 == 0 && b1 % 64 == 0 && b0 <= b1 && b1 <= (long)list.size(), "a section is whole blocks of 64");
    REQUIRE(b1 - b0 == (real + 63) / 64 * 64, "a section is padded to the next block only");
    for (long j = b0; j < b1; ++j)
        if (j - b0 < real) REQUIRE(list[j] >= 0 && list[j] < n, "a real entry is a plan cell");
        else REQUIRE(list[j] == -1, "the padding is -1 only");
    return 0;
}

int main() {
    int nrow, ncol, ng;
    if (std::scanf("%d %d", &nrow, &ncol) != 2) return 1;
    const long n2 = (long)nrow * ncol;
    std::vector<int> fd(n2), act(n2);
    for (long i = 0; i < n2; ++i) if (std::scanf("%d", &fd[i]) != 1) return 1;
    for (long i = 0; i < n2; ++i) if (std::scanf("%d", &act[i]) != 1) return 1;
    if (std::scanf("%d", &ng) != 1) return 1;
    std::vector<int> gpos((size_t)2 * ng);
    for (int i = 0; i < 2 * ng; ++i) if (std::scanf("%d", &gpos[i]) != 1) return 1;
    std::unique_ptr<float[]> flwdst;
    unsigned long lds_limit = 160 * 1024, lds_static = 0;
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "flwdst")) {
            flwdst.reset(new float[n2]);
            for (long i = 0; i < n2; ++i) { unsigned u; if (std::scanf("%u", &u) != 1) return 1; std::memcpy(&flwdst[i], &u, 4); }
        } else if (!std::strcmp(word, "lds")) {
            if (std::scanf("%lu %lu", &lds_limit, &lds_static) != 2) return 1;
        } else return 1;
    }
    std::unique_ptr<signed char[]> grid(new signed char[n2]);          // as smashx_plan_create keeps them
    for (long c = 0; c < n2; ++c) grid[c] = (fd[c] >= 1 && fd[c] <= 8) ? (signed char)fd[c] : 0;

    SxSchedule s;
    const int rc = sx_build_schedule(nrow, ncol, fd.data(), act.data(), ng, gpos.data(), 512, nullptr, s);
    if (rc == -5) {
        s = SxSchedule(); s.nrow = nrow; s.ncol = ncol; s.k_of_flat.assign(n2, -1);
        for (long c = 0; c < n2; ++c) if (act[c] == 1) { s.k_of_flat[c] = (int)s.cell_flat.size(); s.cell_flat.push_back((int)c); }
        s.n = (int)s.cell_flat.size();
    } else if (rc != 0) { std::printf("rc %d: %s\n", rc, s.error.c_str()); return 3; }
    put("cell_flat", s.cell_flat);
    put("gauge_k", s.gauge_k);

    std::string why;
    const SxForest F = sx_forest(s, grid.get(), &why);
    if (!why.empty()) { std::printf("forest_refusal %s\nok\n", why.c_str()); return 0; }
    REQUIRE(rc == 0, "the schedule builder refused a cycle the forest accepts");
    if (check_forest(s, grid.get(), F)) return 2;
    put("up", F.up); put("upn", F.upn); put("parent", F.parent); put("level", F.level); put("order", F.order); put("level_begin", F.level_begin);

    const SxResHost R = sx_res_host_tables(F, s.gauge_k, ng, lds_limit, lds_static);
    if (!R.refusal.empty()) std::printf("res_refusal %s\n", R.refusal.c_str());
    else {
        if (check_res(F, s.gauge_k, ng, R)) return 2;
        std::printf("res_floats %zu\n", R.floats);
        put("res_cell", R.cell); put("res_level", R.level); put("res_upline", R.upline); put("res_upn", R.upn); put("res_ownline", R.ownline);
        put("res_gfirst", R.gfirst); put("res_gnext", R.gnext);
    }

    const SxCatchments C = sx_catchment_lists(s, grid.get(), ng, &why);
    if (!why.empty()) { std::printf("mf_refusal %s\nok\n", why.c_str()); return 0; }
    REQUIRE((int)C.count.size() == ng && (int)C.begin.size() == ng + 1 && C.begin[0] == 0 && C.begin[ng] == (int)C.list.size(), "catchment sizes");
    for (int g = 0; g < ng; ++g) if (check_section(C.list, C.begin[g], C.begin[g + 1], C.count[g], s.n)) return 2;
    put("mf_count", C.count); put("mf_begin", C.begin); put("mf_list", C.list);

    if (flwdst) {
        const SxPiHost P = sx_pi_host_tables(s, C, flwdst.get(), ng, &why);
        if (!why.empty()) { std::printf("pi_refusal %s\nok\n", why.c_str()); return 0; }
        REQUIRE((int)P.gauges.size() == ng && P.entries == (long)P.list.size() && P.dl.size() == P.d2l.size(), "index table sizes");
        long catchment = 0;
        for (int g = 0; g < ng; ++g) {
            const SxPiGauge& G = P.gauges[g];
            REQUIRE(G.sec[0] == 0 && G.lb % 64 == 0 && G.db % 64 == 0 && G.krr >= 0 && G.krr < s.n, "gauge constants");
            const long end = g + 1 < ng ? P.gauges[g + 1].lb : (long)P.list.size();
            REQUIRE(G.lb + 64L * G.sec[SX_PI_NQ] == end, "a gauge's sections fill its part of the list");
            for (int k = 0; k < SX_PI_NQ; ++k) {
                REQUIRE(G.sec[k] <= G.sec[k + 1], "sec is non-decreasing");
                if (check_section(P.list, G.lb + 64L * G.sec[k], G.lb + 64L * G.sec[k + 1], k == 0 ? C.count[g] : (long)G.cnt[k], s.n)) return 2;
            }
            REQUIRE(G.db + 64L * G.sec[1] <= (long)P.dl.size(), "the distances of the catchment lie inside dl");
            catchment += C.count[g];
            std::printf("pi_gauge %d %d %d", G.lb, G.db, G.krr);
            for (int v : G.sec) std::printf(" %d", v);
            for (float v : G.wf) std::printf(" %u", bits(v));
            for (float v : G.cnt) std::printf(" %u", bits(v));
            std::printf("\n");
        }
        REQUIRE(catchment == P.catchment_entries, "catchment entries");
        put("pi_list", P.list); put("pi_dl", P.dl); put("pi_d2l", P.d2l);
    }
    std::printf("ok\n");
    return 0;
}
