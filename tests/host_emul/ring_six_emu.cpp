// tests/host_emul/ring_six_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The six-base ring form of secp256k1_zkp_amd/csrc/ecmult.h (ring6_recode, ecmult_ring6_tables, ecmult_ring6_step) compiled for the host
// (S2K_VERIFY on), next to the three-base form it is checked against: ring_table_prefix_emu.cpp is included as it is, so this library
// carries its own copy of hostemu.cpp's generator table and of the three-base entry points.  The table is a heap vector of exactly
// S2K_RTAB_WORDS words and the parking area one of exactly `park_words` words; ring_six_bounds.cpp runs the same calls under the address
// sanitizer with park_words = W of the six-base parking map.
#include "ring_table_prefix_emu.cpp"

static int r6_put_words(u32* out520, const std::vector<u32>& rtab) {
    fe zi;
    for (int i = 0; i < 9; i++) zi.n[i] = rtab[S2K_RTAB_ZISO + i];
    const int zero = fe_normalizes_to_zero(zi);
    fe_normalize(zi);
    for (int i = 0; i < 512; i++) out520[i] = rtab[i];
    fe_to_words(out520 + 512, zi);
    return zero ? 0 : 1;
}

extern "C" {
int emu_r6_six(void) { return S2K_RING_SIX; }
int emu_r6_sizes(int* out6) {
    out6[0] = S2K_RTAB_WORDS; out6[1] = S2K_RRAW_WAVE_WORDS; out6[2] = 2 * S2K_RING_ENTRIES * 27; out6[3] = S2K_RING_DIG_WORDS;
    out6[4] = S2K_R6_PARK_WORDS; out6[5] = S2K_DIG_WORDS;
    return 6;
}
// the nine digit words of a step from six pieces (order of sc_split_pieces3: C piece of k1, of k2, T1 piece of k1, of k2, T2 piece of k1, of k2)
void emu_r6_recode(u32* dw9, const unsigned long long* m6, const int* neg6) {
    piece43 pc[6];
    for (int s = 0; s < 6; s++) { pc[s].m = (u64)m6[s]; pc[s].neg = neg6[s]; }
    ring6_recode(dw9, pc);
}
// the 32 finished sectors of the table of C (T1 = 2^43 C, T2 = 2^86 C by doublings), every entry taken back to the real curve with the Z
// factor: out = 32 x (x | y) big-endian, in sector order.  Returns 0 when the Z factor is zero.
int emu_r6_table(unsigned char* out2048, const unsigned char* c64, int park_words) {
    gej A, T1, T2; r3_point(A, T1, T2, c64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
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
// the table of C as the kernels build it, as it stands in memory: out520 = the 32 sectors (512 words) and the Z factor, normalised (8 words).
// Returns 0 when the Z factor normalises to zero, 1 otherwise.
int emu_r6_table_words_of(u32* out520, const unsigned char* c64, int park_words) {
    gej A, T1, T2; r3_point(A, T1, T2, c64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
    return r6_put_words(out520, rtab);
}
// the same words for three bases given independently, as affine points (C = T1 and the like can be put in: every dx can be made to vanish)
int emu_r6_table_words(u32* out520, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64, int park_words) {
    gej A, T1, T2; r3p_bases(A, T1, T2, c64, t1_64, t2_64);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
    return r6_put_words(out520, rtab);
}
// R = e*C + s*G + f*G: the six-base form, and when the step hands back (returns 0) the caller's fallback, ecmult_lane on C itself.
// *took = 1 when the ring form produced the result.  zero_ziso != 0: the table's Z factor is overwritten with zero before the step (which
// then has to hand back).  Returns the infinity flag of the result.
int emu_r6_step(unsigned char* r64, int* took, const unsigned char* c64, const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int zero_ziso,
                int park_words) {
    gej A, T1, T2, R; r3_point(A, T1, T2, c64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0);
    std::vector<u32> dig(S2K_RING_DIG_WORDS, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
    if (zero_ziso) for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = 0;
    const int done = ecmult_ring6_step(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig.data());
    if (!done) {
        scalar sf; sc_add(sf, sg, f);
        u32 dig2[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig2};
        ecmult_lane(R, A, e, sf, 1, gtab_host(), lm);
    } else R.inf = 0;
    *took = done;
    return gej_to_b64(r64, R);
}
// a step on the table of three independent bases: returns what ecmult_ring6_step returns (0 = handed back, nothing produced)
int emu_r6_step_bases(unsigned char* r64, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64,
                      const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int park_words) {
    gej A, T1, T2, R; r3p_bases(A, T1, T2, c64, t1_64, t2_64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0), dig(S2K_RING_DIG_WORDS, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
    const int done = ecmult_ring6_step(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig.data());
    memset(r64, 0, 64);
    if (done) { R.inf = 0; gej_to_b64(r64, R); }
    return done;
}
}
