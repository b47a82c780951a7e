// Prints the field table of smash_amd/csrc/sx_fields.h for tests/test_fields_cpu.py: per structure, every slot with its field and
// every field with its slot, whether it is a state and whether its cell vector lives on the routing stream.
#include <cstdio>

#include "../../smash_amd/csrc/sx_fields.h"

int main() {
    std::printf("sizes %d %d %d %d %d\n", SMASHX_GNP, SMASHX_GNS, SX_NFIELDS, SX_NPSLOTS, SX_NSLOTS);
    for (int st = 1; st <= 5; ++st) {
        for (int s = 0; s < SX_NSLOTS; ++s)
            std::printf("slot %d %d %d %d %d\n", st, s, sx_slot_field(st, s), (int)sx_slot_is_state(s), (int)sx_slot_on_routing(s));
        for (int f = 0; f < SX_NFIELDS; ++f)
            std::printf("field %d %d %d %d %d\n", st, f, sx_field_slot(st, f), (int)sx_field_is_state(f), (int)sx_field_on_routing(st, f));
    }
    std::printf("seed");
    for (const int s : SX_SEED_ORDER) std::printf(" %d", s);
    std::printf("\n");
    return 0;
}
