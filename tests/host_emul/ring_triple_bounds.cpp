// tests/host_emul/ring_triple_bounds.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program for the address and undefined-behaviour sanitizers: the construction of the three-base ring table and steps on it,
// with a table of exactly S2K_RTAB_WORDS (528) words and a parking area of exactly 32 x 27 (864) words, both heap vectors, so that a word
// written or read outside the layout that ecmult.h documents is an error the sanitizer reports.  Prints "ok" and returns 0 when every
// step equals the general form's result.
#include "ring_triple_emu.cpp"
#include <stdio.h>

int main() {
    static_assert(S2K_RTAB_WORDS == 528 && 2 * S2K_RING_ENTRIES * 27 == 864 && S2K_RING_DIG_WORDS == 27, "sizes the layout is pinned to");
    unsigned char c64[64], e32[32], s32[32], f32[32], got[64], want[64];
    {   // C = 5 G
        ge g; ge_set_generator(g); gej j, t; gej_set_ge(j, g);
        gej_double(t, j); j = t; gej_double(t, j); j = t; gej_add_ge(t, j, g);
        if (gej_to_b64(c64, t)) return 2;
    }
    unsigned x = 0x9E3779B9u;
    for (int round = 0; round < 4; round++) {
        for (int i = 0; i < 32; i++) { x = x * 1664525u + 1013904223u; e32[i] = (unsigned char)(x >> 24); x = x * 1664525u + 1013904223u; s32[i] = (unsigned char)(x >> 24);
                                       x = x * 1664525u + 1013904223u; f32[i] = (unsigned char)(x >> 24); }
        e32[0] &= 0x7F; s32[0] &= 0x7F; f32[0] &= 0x7F;
        int took = -1;
        if (emu_r3_step(got, &took, c64, e32, s32, f32, 0) || took != 1) { printf("step %d: infinity or handed back (%d)\n", round, took); return 1; }
        if (emu_r3_step(want, &took, c64, e32, s32, f32, 1) || took != 0) { printf("step %d: zero Z factor not handed back (%d)\n", round, took); return 1; }
        if (memcmp(got, want, 64)) { printf("step %d: differs from the general form\n", round); return 1; }
    }
    unsigned char tab[2048];
    if (emu_r3_table(tab, c64) != 1) return 3;
    printf("ok\n");
    return 0;
}
