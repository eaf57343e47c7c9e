// tests/host_emul/ring_triple_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The three-base ring form of secp256k1_zkp_amd/csrc/ecmult.h (ecmult_ring3_tables, ecmult_ring3_step and its recoding) compiled for the
// host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit digits): that file is included as it is, so this
// library carries its own copy of the table and is loaded next to libs2k_hostemu.so.  The table and the parking area are heap vectors of
// exactly S2K_RTAB_WORDS and 32 x 27 words: ring_triple_bounds.cpp runs the same two calls under the address sanitizer.
#include "hostemu.cpp"

static void r3_point(gej& A, gej& T1, gej& T2, const unsigned char* c64) {
    ge a; ge_from_b64(a, c64); fe_norm_weak(a.x); fe_norm_weak(a.y);
    gej_set_ge(A, a);
    T2 = A;
    for (int k = 0; k < 86; k++) {
        if (k == 43) { T1 = T2; fe_norm_weak(T1.y); }
        gej_double_lean(T2, T2);
    }
    fe_norm_weak(T2.y);
}

extern "C" {
int emu_r3_triple(void) { return S2K_RING_TRIPLE; }
int emu_r3_sizes(int* out4) { out4[0] = S2K_RTAB_WORDS; out4[1] = S2K_RRAW_WAVE_WORDS; out4[2] = 2 * S2K_RING_ENTRIES * 27; out4[3] = S2K_RING_DIG_WORDS; return 4; }
// the 22 signed digits d_i = 2 b_i - 3 (i = 0 least significant) of an odd piece magnitude <= 2^44 - 1
void emu_r3_piece_digits(int* out22, unsigned long long m) {
    for (int i = 0; i < S2K_R3_DIGITS; i++) out22[i] = 2 * (int)ring3_piece_field((u64)m, i) - 3;
}
unsigned emu_r3_field(unsigned vc, unsigned v1, unsigned v2, unsigned sc, unsigned s1, unsigned s2) { return ring3_field(vc, v1, v2, sc, s1, s2); }
// the nine digit words of a step from six pieces (order of sc_split_pieces3: C piece of k1, of k2, T1 piece of k1, of k2, T2 piece of k1, of k2)
void emu_r3_recode(u32* dw9, const unsigned long long* m6, const int* neg6) {
    piece43 pc[6];
    for (int s = 0; s < 6; s++) { pc[s].m = (u64)m6[s]; pc[s].neg = neg6[s]; }
    ring3_recode(dw9, pc);
}
static void r3_put_pieces(unsigned long long* m6, int* neg6, u32* hw10, int* hneg2, const half_scalar& h0, const half_scalar& h1) {
    piece43 pc[6]; sc_split_pieces3(pc, h0, h1);
    for (int s = 0; s < 6; s++) { m6[s] = pc[s].m; neg6[s] = pc[s].neg; }
    for (int i = 0; i < 5; i++) { hw10[i] = h0.w[i]; hw10[5 + i] = h1.w[i]; }
    hneg2[0] = h0.neg; hneg2[1] = h1.neg;
}
// the six pieces of e as ecmult_ring3_step cuts them, and the two odd GLV halves they were cut from (5 words and a sign each)
void emu_r3_pieces(unsigned long long* m6, int* neg6, u32* hw10, int* hneg2, const unsigned char* e32) {
    scalar e; sc_set_b32(e, e32, nullptr);
    half_scalar h0, h1; sc_split_lambda_odd(h0, h1, e);
    r3_put_pieces(m6, neg6, hw10, hneg2, h0, h1);
}
// the same cut of two given halves (odd magnitudes below 2^129: 5 words and a sign each)
void emu_r3_pieces_of_halves(unsigned long long* m6, int* neg6, const u32* hw10, const int* hneg2) {
    half_scalar h0, h1;
    for (int i = 0; i < 5; i++) { h0.w[i] = hw10[i]; h1.w[i] = hw10[5 + i]; }
    h0.neg = hneg2[0]; h1.neg = hneg2[1];
    u32 hw[10]; int hn[2];
    r3_put_pieces(m6, neg6, hw, hn, h0, h1);
}
// the 32 finished sectors of the table of C (T1 = 2^43 C, T2 = 2^86 C by doublings), every entry taken back to the real curve with the Z
// factor: out = 32 x (x | y) big-endian, in sector order.  Returns 0 when the Z factor is zero.
int emu_r3_table(unsigned char* out2048, const unsigned char* c64) {
    gej A, T1, T2; r3_point(A, T1, T2, c64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw(2 * S2K_RING_ENTRIES * 27, 0);
    ecmult_ring3_tables(rtab.data(), rraw.data(), A, T1, T2);
    fe zi;
    for (int i = 0; i < 9; i++) zi.n[i] = rtab[S2K_RTAB_ZISO + i];
    if (fe_normalizes_to_zero(zi)) return 0;
    for (int en = 0; en < 32; en++) {
        gej J; J.inf = 0; J.z = zi;
        fe_from_words(J.x, rtab.data() + 16 * en); fe_from_words(J.y, rtab.data() + 16 * en + 8);
        gej_to_b64(out2048 + 64 * en, J);
    }
    return 1;
}
// R = e*C + s*G + f*G: the three-base form, and when the step hands back (returns 0) the caller's fallback, ecmult_lane on C itself.
// *took = 1 when the ring form produced the result.  zero_ziso != 0: the table's Z factor is overwritten with zero before the step (which
// then has to hand back).  Returns the infinity flag of the result.
int emu_r3_step(unsigned char* r64, int* took, const unsigned char* c64, const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int zero_ziso) {
    gej A, T1, T2, R; r3_point(A, T1, T2, c64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw(2 * S2K_RING_ENTRIES * 27, 0);
    std::vector<u32> dig(S2K_RING_DIG_WORDS, 0);
    ecmult_ring3_tables(rtab.data(), rraw.data(), A, T1, T2);
    if (zero_ziso) for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = 0;
    const int done = ecmult_ring3_step(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig.data());
    if (!done) {
        scalar sf; sc_add(sf, sg, f);
        u32 dig2[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig2};
        ecmult_lane(R, A, e, sf, 1, gtab_host(), lm);
    } else R.inf = 0;
    *took = done;
    return gej_to_b64(r64, R);
}
}
