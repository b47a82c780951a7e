// sx_fields.h -- the one table of model fields: which of the 24 fields of smashx_parameters / smashx_states each structure reads,
// and which of the 14 per-cell device vectors (slots) holds it.  Plain C++17, no device pointers: the host driver (smashx.hip,
// slot_vecs) turns a slot into its vectors, a CPU program can include this file alone (tests/csrc/sx_fields_check.cpp).
//
// Fields are numbered as the regulariser, the control vector and the ensemble path number them: 0..15 = SMASHX_P_*, 16..23 =
// SMASHX_GNP + SMASHX_S_* (parameters, then states).  Slots: 0..8 hold parameters -- ci, cp, cft, cst, exc, lr, px[0..2] of
// SxDeviceArrays; vic-a puts b, cusl1, cusl2, clsl, ks in 0..4 and ds, dsm, ws in px -- and 9..13 hold states -- hi, hp, hft, hst, hlr;
// vic-a: husl1, husl2, hlsl in 9..11.  (smash/core/_constant.py:15-29; ci via gr_interception.)
#pragma once
#include "../../include/smashx.h"

constexpr int SX_NFIELDS = SMASHX_GNP + SMASHX_GNS;
constexpr int SX_NPSLOTS = 9, SX_NSSLOTS = 5, SX_NSLOTS = SX_NPSLOTS + SX_NSSLOTS;
// the slots by name (the GR names; vic-a's occupants are listed above)
enum : int { SX_SLOT_CI, SX_SLOT_CP, SX_SLOT_CFT, SX_SLOT_CST, SX_SLOT_EXC, SX_SLOT_LR, SX_SLOT_PX0, SX_SLOT_PX1, SX_SLOT_PX2,
             SX_SLOT_HI, SX_SLOT_HP, SX_SLOT_HFT, SX_SLOT_HST, SX_SLOT_HLR };
static_assert(SX_SLOT_PX2 + 1 == SX_NPSLOTS && SX_SLOT_HLR + 1 == SX_NSLOTS, "14 names for 14 slots");

#define SX_F_P(name) SMASHX_P_##name
#define SX_F_S(name) (SMASHX_GNP + SMASHX_S_##name)
// slot -> field, per structure (1 gr-a, 2 gr-b, 3 gr-c, 4 gr-d, 5 vic-a); -1: the structure leaves the slot unused
constexpr int SX_SLOT_FIELD[5][SX_NSLOTS] = {
    {-1, SX_F_P(CP), SX_F_P(CFT), -1, SX_F_P(EXC), SX_F_P(LR), -1, -1, -1,
     -1, SX_F_S(HP), SX_F_S(HFT), -1, SX_F_S(HLR)},
    {SX_F_P(CI), SX_F_P(CP), SX_F_P(CFT), -1, SX_F_P(EXC), SX_F_P(LR), -1, -1, -1,
     SX_F_S(HI), SX_F_S(HP), SX_F_S(HFT), -1, SX_F_S(HLR)},
    {SX_F_P(CI), SX_F_P(CP), SX_F_P(CFT), SX_F_P(CST), SX_F_P(EXC), SX_F_P(LR), -1, -1, -1,
     SX_F_S(HI), SX_F_S(HP), SX_F_S(HFT), SX_F_S(HST), SX_F_S(HLR)},
    {-1, SX_F_P(CP), SX_F_P(CFT), -1, -1, SX_F_P(LR), -1, -1, -1,
     -1, SX_F_S(HP), SX_F_S(HFT), -1, SX_F_S(HLR)},
    {SX_F_P(B), SX_F_P(CUSL1), SX_F_P(CUSL2), SX_F_P(CLSL), SX_F_P(KS), SX_F_P(LR), SX_F_P(DS), SX_F_P(DSM), SX_F_P(WS),
     SX_F_S(HUSL1), SX_F_S(HUSL2), SX_F_S(HLSL), -1, SX_F_S(HLR)},
};
#undef SX_F_P
#undef SX_F_S

inline bool sx_field_is_state(int field) { return field >= SMASHX_GNP; }
inline bool sx_slot_is_state(int slot) { return slot >= SX_NPSLOTS; }
// the routing parameter and the routing store: their cell vectors are read and written on the routing stream, every other slot's on
// the stream of the vertical kernels
inline bool sx_slot_on_routing(int slot) { return slot == SX_SLOT_LR || slot == SX_SLOT_HLR; }
inline int sx_slot_field(int st, int slot) { return SX_SLOT_FIELD[st - 1][slot]; }
inline int sx_field_slot(int st, int field) {
    for (int s = 0; s < SX_NSLOTS; ++s) if (SX_SLOT_FIELD[st - 1][s] == field) return s;
    return -1;
}
inline bool sx_field_on_routing(int st, int field) { const int s = sx_field_slot(st, field); return s >= 0 && sx_slot_on_routing(s); }

// The order in which an adjoint sweep seeds the 14 gradient vectors: the reservoirs' parameters and levels, the routing pair, px.
// (Within a stream the seeds are queued in this order; it is not the ascending one, and stays as the sweeps have always queued them.)
constexpr int SX_SEED_ORDER[SX_NSLOTS] = {0, 1, 2, 3, 4, 9, 10, 11, 12, SX_SLOT_LR, SX_SLOT_HLR, 6, 7, 8};
