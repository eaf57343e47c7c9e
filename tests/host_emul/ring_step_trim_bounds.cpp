// tests/host_emul/ring_step_trim_bounds.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program for the address and undefined-behaviour sanitizers: steps of the six-base ring form on the signed-accumulator forms,
// the point returned as fractions, with the table, the parking area and the digit area heap vectors of exactly their declared sizes
// (S2K_RTAB_WORDS, W = 243, S2K_RING_DIG_WORDS = 27), against the general form.  Prints "ok" and returns 0 when every step agrees.
#include "ring_step_trim_emu.cpp"
#include <stdio.h>

int main() {
    static_assert(S2K_RTAB_WORDS == 528 && S2K_RING_DIG_WORDS == 27 && S2K_R6_PARK_WORDS == 243, "sizes the layout is pinned to");
    unsigned char c64[64], e32[32], s32[32], f32[32], got[64], want[64];
    {   // C = 5 G
        ge g; ge_set_generator(g); gej j, t; gej_set_ge(j, g);
        gej_double(t, j); j = t; gej_double(t, j); j = t; gej_add_ge(t, j, g);
        if (gej_to_b64(c64, t)) return 2;
    }
    unsigned x = 0x51ED270Bu;
    for (int round = 0; round < 3; round++) {
        for (int i = 0; i < 32; i++) { x = x * 1664525u + 1013904223u; e32[i] = (unsigned char)(x >> 24); x = x * 1664525u + 1013904223u; s32[i] = (unsigned char)(x >> 24);
                                       x = x * 1664525u + 1013904223u; f32[i] = (unsigned char)(x >> 24); }
        e32[0] &= 0x7F; s32[0] &= 0x7F; f32[0] &= 0x7F;
        if (emu_trim_step(got, c64, e32, s32, f32, S2K_R6_PARK_WORDS) != 1) { printf("step %d: handed back\n", round); return 1; }
        int took = -1;                                                          // the general form: the hand-back path of emu_r6_step (Z factor zeroed)
        if (emu_r6_step(want, &took, c64, e32, s32, f32, 1, S2K_R6_PARK_WORDS) || took != 0) { printf("step %d: zero Z factor not handed back (%d)\n", round, took); return 1; }
        if (memcmp(got, want, 64)) { printf("step %d: differs from the general form\n", round); return 1; }
    }
    printf("ok\n");
    return 0;
}
