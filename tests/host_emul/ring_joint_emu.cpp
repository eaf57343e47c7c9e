// tests/host_emul/ring_joint_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The ring form of secp256k1_zkp_amd/csrc/ecmult.h (ecmult_ring_tables, ecmult_ring_step and the joint form's recoding) compiled for the
// host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit digits): that file is included as it is, so this
// library carries its own copy of the table and is loaded next to libs2k_hostemu.so.  Built twice: as it is (the joint table) and with
// -DS2K_RING_JOINT=0 (the two separate tables, the control).
#include "hostemu.cpp"

static void rj_point(gej& A, gej& T, const unsigned char* c64) {
    ge a; ge_from_b64(a, c64); fe_norm_weak(a.x); fe_norm_weak(a.y);
    gej_set_ge(A, a);
    T = A; for (int k = 0; k < 64; k++) gej_double_lean(T, T);
    fe_norm_weak(T.y);
}

extern "C" {
int emu_rj_joint(void) { return S2K_RING_JOINT; }
int emu_rj_adds(void) { return S2K_RING_ADDS_P; }
int emu_rj_sizes(int* out4) { out4[0] = S2K_RTAB_WORDS; out4[1] = S2K_RRAW_WAVE_WORDS; out4[2] = 2 * S2K_RING_ENTRIES * 27; out4[3] = S2K_RING_DIG_WORDS; return 4; }
#if S2K_RING_JOINT
// the 22 signed digits d_i = 2 b_i - 7 (i = 0 least significant) of the odd piece w[0] + 2^32 w[1] + 2^64 w[2] < 2^65
void emu_rj_piece_digits(int* out22, const u32* w3) {
    piece65 p; p.w[0] = w3[0]; p.w[1] = w3[1]; p.w[2] = w3[2]; p.neg = 0;
    for (int i = 0; i < S2K_RING_DIGITS; i++) out22[i] = 2 * (int)ring_piece_field(p, i) - 7;
}
unsigned emu_rj_field(unsigned vc, unsigned vt, unsigned sc, unsigned st) { return ring_joint_field(vc, vt, sc, st); }
// the nine digit words of a step from four pieces (stream order of sc_split_pieces: C piece of k1, of k2, T piece of k1, of k2)
void emu_rj_recode(u32* dw9, const u32* w12, const int* neg4) {
    piece65 pc[4];
    for (int s = 0; s < 4; s++) { for (int i = 0; i < 3; i++) pc[s].w[i] = w12[3 * s + i]; pc[s].neg = neg4[s]; }
    ring_joint_recode(dw9, pc);
}
#endif
// the four pieces of e as ecmult_ring_step cuts them: w12 = 4 x 3 words, neg4 = their signs
void emu_rj_pieces(u32* w12, int* neg4, const unsigned char* e32) {
    scalar e; sc_set_b32(e, e32, nullptr);
    half_scalar h0, h1; sc_split_lambda_odd(h0, h1, e);
    piece65 pc[4]; sc_split_pieces(pc, h0, h1);
    for (int s = 0; s < 4; s++) { for (int i = 0; i < 3; i++) w12[3 * s + i] = pc[s].w[i]; neg4[s] = pc[s].neg; }
}
// the 32 finished sectors of the tables of C (T = 2^64 C by 64 doublings), every entry taken back to the real curve with the Z factor:
// out = 32 x (x | y) big-endian, in sector order.  Returns 0 when the Z factor is zero.
int emu_rj_table(unsigned char* out2048, const unsigned char* c64) {
    gej A, T; rj_point(A, T, c64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw(2 * S2K_RING_ENTRIES * 27, 0);
    ecmult_ring_tables(rtab.data(), rraw.data(), A, T);
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
// R = e*C + s*G + f*G as prim 40 of tests/gpu_prims/prims.hip runs it: the ring form, and when the step hands back (returns 0) the
// caller's fallback, ecmult_lane on C itself.  *took = 1 when the ring form produced the result.  zero_ziso != 0: the table's Z factor
// is overwritten with zero before the step (which then has to hand back).  Returns the infinity flag of the result.
int emu_rj_step(unsigned char* r64, int* took, const unsigned char* c64, const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int zero_ziso) {
    gej A, T, R; rj_point(A, T, c64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw(2 * S2K_RING_ENTRIES * 27, 0);
    u32 dig[S2K_RING_DIG_WORDS];
    ecmult_ring_tables(rtab.data(), rraw.data(), A, T);
    if (zero_ziso) for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = 0;
    const int done = ecmult_ring_step(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig);
    if (!done) {
        scalar sf; sc_add(sf, sg, f);
        u32 dig2[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig2};
        ecmult_lane(R, A, e, sf, 1, gtab_host(), lm);
    } else R.inf = 0;
    *took = done;
    return gej_to_b64(r64, R);
}
}
