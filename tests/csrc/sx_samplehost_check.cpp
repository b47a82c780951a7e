// sx_samplehost_check.cpp -- the plain-C++ host side of the two sample paths (smash_amd/csrc/sx_samplehost.h): the field map of every
// structure, the staging of every batch of a sample and the batch / time-chunk choice, every buffer a heap block of exactly the size the
// library's caller owes: built with -fsanitize=address,undefined by tests/test_sample_host_sanitized.py.
// argv: nfields nsamples SP.  Prints "ok <batches>" or "VIOLATION ...".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../smash_amd/csrc/sx_samplehost.h"

#define VIOLATION(...) do { printf("VIOLATION " __VA_ARGS__); puts(""); return 1; } while (0)

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int nfields = atoi(argv[1]), nsamples = atoi(argv[2]), SP = atoi(argv[3]);

    // staging: column c of batch b holds sample min(b * SP + c, nsamples - 1); sample value = 1000 * sample + field
    std::unique_ptr<float[]> sample(new float[(size_t)nfields * nsamples + (nfields == 0)]);
    for (int s = 0; s < nsamples; ++s)
        for (int j = 0; j < nfields; ++j) sample[(size_t)j + (size_t)nfields * s] = 1000.f * s + j;
    const int nbatch = (nsamples + SP - 1) / SP;
    for (int b = 0; b < nbatch; ++b) {
        const size_t len = (size_t)(nfields > 0 ? nfields : 1) * SP;      // what the driver allocates: max(nfields, 1) * SP
        std::unique_ptr<float[]> hs(new float[len]);
        for (size_t i = 0; i < len; ++i) hs[i] = -1.f;
        sx_sh_stage(nfields > 0 ? sample.get() : nullptr, nfields, nsamples, b * SP, SP, hs.get());
        for (int j = 0; j < nfields; ++j)
            for (int c = 0; c < SP; ++c) {
                const int s = b * SP + c < nsamples - 1 ? b * SP + c : nsamples - 1;
                if (hs[(size_t)j * SP + c] != 1000.f * s + j) VIOLATION("stage: batch %d field %d column %d holds %g", b, j, c, hs[(size_t)j * SP + c]);
            }
        if (nfields == 0)
            for (int c = 0; c < SP; ++c) if (hs[c] != -1.f) VIOLATION("stage: wrote without a field");
    }

    // field map: per structure, every field it uses lands in its slot, every other is refused; 0, 25 and a repeat are refused
    for (int st = 1; st <= 5; ++st) {
        int smap[SX_NSLOTS];
        if (!sx_sh_field_map(st, 0, nullptr, smap).empty()) VIOLATION("map: nfields = 0 refused");
        for (int s = 0; s < SX_NSLOTS; ++s) if (smap[s] != -1) VIOLATION("map: nfields = 0 maps slot %d", s);
        for (int f = 1; f <= SX_NFIELDS; ++f) {
            int slot = -1;
            for (int s = 0; s < SX_NSLOTS; ++s) if (SX_SLOT_FIELD[st - 1][s] == f - 1) slot = s;
            std::unique_ptr<int[]> one(new int[1]), twice(new int[2]);
            one[0] = twice[0] = twice[1] = f;
            const std::string why = sx_sh_field_map(st, 1, one.get(), smap);
            if (slot >= 0) {
                if (!why.empty()) VIOLATION("map: structure %d refuses its field %d: %s", st, f, why.c_str());
                for (int s = 0; s < SX_NSLOTS; ++s) if (smap[s] != (s == slot ? 0 : -1)) VIOLATION("map: structure %d field %d slot %d = %d", st, f, s, smap[s]);
                if (!has(sx_sh_field_map(st, 2, twice.get(), smap), "is listed twice")) VIOLATION("map: structure %d takes field %d twice", st, f);
            } else if (!has(why, "is not used by the structure")) VIOLATION("map: structure %d takes field %d: '%s'", st, f, why.c_str());
        }
        for (int bad : {0, 25, -3}) {
            std::unique_ptr<int[]> one(new int[1]);
            one[0] = bad;
            if (!has(sx_sh_field_map(st, 1, one.get(), smap), "is outside 1..24")) VIOLATION("map: structure %d takes index %d", st, bad);
        }
    }

    // batch and time chunk (n = 144 cells, nt = 48 steps, 2 gauges)
    const double GiB = 1024.0 * 1024 * 1024;
    int sp = 0, tc = 0;
    sx_sh_budget(144, 48, 2, nsamples, true, 0, 0, 64 * GiB, 0.0, &sp, &tc);
    if (sp != std::min((nsamples + 63) / 64 * 64, 16384) || tc != 48) VIOLATION("budget: a fitting one gives (%d, %d)", sp, tc);
    sx_sh_budget(1 << 20, 1 << 20, 2, 1 << 20, true, 0, 0, 1024.0, 0.0, &sp, &tc);
    if (sp != 64 || tc != 256) VIOLATION("budget: too small a one ends at (%d, %d)", sp, tc);
    sx_sh_budget(1 << 20, 1 << 20, 2, 1 << 20, false, 640, 1000, 1024.0, 0.0, &sp, &tc);
    if (sp != 640 || tc != 1000) VIOLATION("budget: forced lengths give (%d, %d)", sp, tc);
    sx_sh_budget(144, 48, 2, 1 << 20, false, 1, 0, 64 * GiB, 0.0, &sp, &tc);
    if (sp != 64 || tc != 48) VIOLATION("budget: a forced batch of 1 gives (%d, %d)", sp, tc);
    printf("ok %d\n", nbatch);
    return 0;
}
