// sx_samplehost.h -- the host side of the two sample paths (smashx_multiple_run, smashx_uniform_costs; smashx.hip) that is plain C++17:
// the map from the caller's field list to the slots, the staging of one batch of the sample, the batch and time-chunk lengths of the
// ensemble path.  No device pointer and no HIP call: a CPU program can include this file alone (tests/csrc/sx_samplehost_check.cpp
// runs it under AddressSanitizer + UndefinedBehaviorSanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "sx_fields.h"

// ind[j] in 1..24 names the field that row j of the sample replaces -> smap[slot] = j, -1 for a slot that keeps its base field.
// "": fine; else the reason the caller returns SMASHX_E_ARG with, behind its own name
inline std::string sx_sh_field_map(int st, int nfields, const int* ind, int smap[SX_NSLOTS]) {
    for (int s = 0; s < SX_NSLOTS; ++s) smap[s] = -1;
    for (int j = 0; j < nfields; ++j) {
        const int f = ind[j];
        if (f < 1 || f > SX_NFIELDS) return "ind_parameters_states[" + std::to_string(j) + "] = " + std::to_string(f) + " is outside 1..24";
        const int slot = sx_field_slot(st, f - 1);
        if (slot < 0) return "field " + std::to_string(f) + " is not used by the structure";
        if (smap[slot] >= 0) return "field " + std::to_string(f) + " is listed twice";
        smap[slot] = j;
    }
    return "";
}

// sample (nfields, nsamples) column-major -> hs[field][column] of the batch that starts at sample s0, SP columns a field; the columns
// past the batch's last sample repeat it (whole wavefronts of ordinary values: nothing of them is ever copied out)
inline void sx_sh_stage(const float* sample, int nfields, int nsamples, int s0, int SP, float* hs) {
    const int cnt = std::min(SP, nsamples - s0);
    for (int j = 0; j < nfields; ++j)
        for (int c = 0; c < SP; ++c) hs[(size_t)j * SP + c] = sample[(size_t)j + (size_t)nfields * (s0 + std::min(c, cnt - 1))];
}

// samples per batch (a multiple of 64) and steps per time chunk of smashx_multiple_run: 16384 and 32768 at the most, halved in turn
// (the chunk first, down to 256, then the batch, down to 64) until the buffers fit 0.6 of the free and the already held bytes, 24 GiB
// at the most.  force_batch / force_chunk > 0 fix a length (SMASHX_ENS_BATCH / SMASHX_ENS_CHUNK)
inline void sx_sh_budget(int n, int nt, int ng, int nsamples, bool want_qsim, int force_batch, int force_chunk, double free_bytes,
                         double held_bytes, int* SP_out, int* Tc_out) {
    int SP = std::min((nsamples + 63) / 64 * 64, force_batch > 0 ? (force_batch + 63) / 64 * 64 : 16384);
    int Tc = std::min(nt, force_chunk > 0 ? force_chunk : 32768);
    const double budget = std::min(0.6 * (free_bytes + held_bytes), 24.0 * 1024 * 1024 * 1024);
    auto need = [&](int sp, int tc) {
        return 4.0 * sp * ((double)n * tc + (double)nt * std::max(ng, 1) * (want_qsim ? 2 : 1) + 5.0 * n + 64.0);
    };
    while (need(SP, Tc) > budget) {
        if (force_chunk == 0 && Tc > 256) Tc = (Tc + 1) / 2;
        else if (force_batch == 0 && SP > 64) SP = (SP / 2 + 63) / 64 * 64;
        else break;      // forced lengths that do not fit: the allocation says so
    }
    *SP_out = SP; *Tc_out = Tc;
}
