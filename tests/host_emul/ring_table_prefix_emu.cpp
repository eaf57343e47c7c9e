// tests/host_emul/ring_table_prefix_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The construction of the three-base ring table (secp256k1_zkp_amd/csrc/ecmult.h: ecmult_ring3_tables) on the host with its three bases
// given INDEPENDENTLY, as affine points: ring_triple_emu.cpp derives T1 and T2 from C by doublings, where no dx of a conjugate pair can
// vanish; here C = T1 + T2 and the like can be put in, so every place where the prefix chain of the dx can break is reachable.  The
// parking area is a heap vector of exactly `park_words` words, the table one of exactly S2K_RTAB_WORDS.
#include "ring_triple_emu.cpp"

static void r3p_bases(gej& A, gej& T1, gej& T2, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64) {
    const unsigned char* in[3] = {c64, t1_64, t2_64};
    gej* out[3] = {&A, &T1, &T2};
    for (int i = 0; i < 3; i++) {
        ge a; ge_from_b64(a, in[i]); fe_norm_weak(a.x); fe_norm_weak(a.y);
        gej_set_ge(*out[i], a);
    }
}

extern "C" {
// the table of (C, T1, T2): out520 = the 32 finished sectors as they stand in the table (512 words) and the Z factor, normalised (8 words).
// Returns 0 when the Z factor normalises to zero, 1 otherwise.
int emu_r3p_table(u32* out520, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64, int park_words) {
    gej A, T1, T2; r3p_bases(A, T1, T2, c64, t1_64, t2_64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    ecmult_ring3_tables(rtab.data(), rraw.data(), A, T1, T2);
    fe zi;
    for (int i = 0; i < 9; i++) zi.n[i] = rtab[S2K_RTAB_ZISO + i];
    const int zero = fe_normalizes_to_zero(zi);
    fe_normalize(zi);
    for (int i = 0; i < 512; i++) out520[i] = rtab[i];
    fe_to_words(out520 + 512, zi);
    return zero ? 0 : 1;
}
// the same words for the table of C as the kernels build it: T1 = 2^43 C and T2 = 2^86 C by lean doublings, on their own Z
int emu_r3p_table_of(u32* out520, const unsigned char* c64, int park_words) {
    gej A, T1, T2; r3_point(A, T1, T2, c64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    ecmult_ring3_tables(rtab.data(), rraw.data(), A, T1, T2);
    fe zi;
    for (int i = 0; i < 9; i++) zi.n[i] = rtab[S2K_RTAB_ZISO + i];
    const int zero = fe_normalizes_to_zero(zi);
    fe_normalize(zi);
    for (int i = 0; i < 512; i++) out520[i] = rtab[i];
    fe_to_words(out520 + 512, zi);
    return zero ? 0 : 1;
}
// a step R = e*C + s*G + f*G on the table of (C, T1, T2): returns what ecmult_ring3_step returns (0 = handed back, nothing produced);
// r64 = the result when it completed
int emu_r3p_step(unsigned char* r64, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64,
                 const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int park_words) {
    gej A, T1, T2, R; r3p_bases(A, T1, T2, c64, t1_64, t2_64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0), dig(S2K_RING_DIG_WORDS, 0);
    ecmult_ring3_tables(rtab.data(), rraw.data(), A, T1, T2);
    const int done = ecmult_ring3_step(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig.data());
    memset(r64, 0, 64);
    if (done) { R.inf = 0; gej_to_b64(r64, R); }
    return done;
}
}
