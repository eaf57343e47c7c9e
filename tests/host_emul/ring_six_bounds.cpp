// tests/host_emul/ring_six_bounds.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program for the address and undefined-behaviour sanitizers: the construction of the six-base ring table with a table of
// exactly S2K_RTAB_WORDS (528) words and a parking area of exactly W = 243 words -- the highest used word + 1 of the parking map that
// ecmult.h documents above S2K_R6_LEVELS -- both heap vectors, so that a word written or read outside that map is an error the sanitizer
// reports; then four steps on that table against the general form.  Prints "ok" and returns 0 when every step agrees.
#include "ring_six_emu.cpp"
#include <stdio.h>

#define R6_PARK_WORDS 243

int main() {
    static_assert(S2K_RTAB_WORDS == 528 && S2K_RING_DIG_WORDS == 27 && S2K_R6_PARK_WORDS == R6_PARK_WORDS, "sizes the layout is pinned to");
    unsigned char c64[64], t1[64], t2[64], e32[32], s32[32], f32[32], got[64], want[64];
    {   // C = 5 G, T1 = 2^43 C, T2 = 2^86 C
        ge g; ge_set_generator(g); gej j, t; gej_set_ge(j, g);
        gej_double(t, j); j = t; gej_double(t, j); j = t; gej_add_ge(t, j, g);
        if (gej_to_b64(c64, t)) return 2;
        for (int k = 0; k < 86; k++) {
            if (k == 43 && gej_to_b64(t1, t)) return 2;
            gej_double(j, t); t = j;
        }
        if (gej_to_b64(t2, t)) return 2;
    }
    u32 words[520];
    if (emu_r6_table_words(words, c64, t1, t2, R6_PARK_WORDS) != 1) { printf("the Z factor of an honest table is zero\n"); return 3; }
    unsigned x = 0x9E3779B9u;
    for (int round = 0; round < 4; round++) {
        for (int i = 0; i < 32; i++) { x = x * 1664525u + 1013904223u; e32[i] = (unsigned char)(x >> 24); x = x * 1664525u + 1013904223u; s32[i] = (unsigned char)(x >> 24);
                                       x = x * 1664525u + 1013904223u; f32[i] = (unsigned char)(x >> 24); }
        e32[0] &= 0x7F; s32[0] &= 0x7F; f32[0] &= 0x7F;
        if (emu_r6_step_bases(got, c64, t1, t2, e32, s32, f32, R6_PARK_WORDS) != 1) { printf("step %d: handed back\n", round); return 1; }
        int took = -1;                                                          // the general form: the hand-back path of emu_r6_step (Z factor zeroed)
        if (emu_r6_step(want, &took, c64, e32, s32, f32, 1, R6_PARK_WORDS) || took != 0) { printf("step %d: zero Z factor not handed back (%d)\n", round, took); return 1; }
        if (memcmp(got, want, 64)) { printf("step %d: differs from the general form\n", round); return 1; }
    }
    if (emu_r6_table_words(words, c64, c64, t2, R6_PARK_WORDS) != 0) { printf("T1 = C: the Z factor is not zero\n"); return 4; }      // a dx of zero, same bounds
    printf("ok\n");
    return 0;
}
