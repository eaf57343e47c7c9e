// tests/host_emul/ring_step_trim_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The signed-accumulator forms of the six-base ring step (secp256k1_zkp_amd/csrc/group.h: gej_dblneg_ring, gej_rsub_ge_ring,
// gez_add_ge_ring) compiled for the host (S2K_VERIFY on, so a limb that would wrap aborts), each next to the shared lean form it
// replaces, and the step that returns its point as fractions (ecmult.h: ecmult_ring6_step_frac).  ring_six_emu.cpp is included as it is.
// Coordinates come in as raw limbs (9 words each), so that a caller can put every limb at the contract's maximum for its magnitude.
// ring_step_trim_prims.hip runs the same three wrappers (trim_*) on the device.
#include "ring_six_emu.cpp"

#include "../gpu_prims/ring_step_trim_forms.h"

extern "C" {
// in: 27 words (x, y, z) as the NEW form takes them (x holds -X when nx).  out_new: its result, 27 words limb for limb.  out_cmp: 6 x 32
// bytes = (X3, Y3, Z3) of the point the new form stands for, then (X3, Y3, Z3) of gej_double_lean on the same point, all canonical.
void emu_trim_dbl(u32* out_new, unsigned char* out_cmp, const u32* in, int nx) {
    gej a, r, s; trim_load(a.x, in); trim_load(a.y, in + 9); trim_load(a.z, in + 18); a.inf = 0;
    trim_dbl(r, a, nx);
    trim_store(out_new, r.x); trim_store(out_new + 9, r.y); trim_store(out_new + 18, r.z);
    fe t;
    fe_to_b32(out_cmp, r.x);
    fe_neg(t, r.y, 1); fe_to_b32(out_cmp + 32, t);                              // r = -2a
    fe_to_b32(out_cmp + 64, r.z);
    s = a;
    if (nx) { fe_neg(s.x, a.x, 2); }
    fe_normalize(s.x); fe_normalize(s.y); fe_normalize(s.z);                    // the shared form's contract: X 1, Y <= 2, Z 1
    gej_double_lean(s, s);
    fe_to_b32(out_cmp + 96, s.x); fe_to_b32(out_cmp + 128, s.y); fe_to_b32(out_cmp + 160, s.z);
}
// in: 45 words (x = +X1, y = -Y1, z, then the operand's x, y).  Returns the new form's same-x flag | 2 * the shared form's.
int emu_trim_rsub(u32* out_new, unsigned char* out_cmp, const u32* in) {
    gej a, r, s; ge b; trim_load(a.x, in); trim_load(a.y, in + 9); trim_load(a.z, in + 18); a.inf = 0; trim_load(b.x, in + 27); trim_load(b.y, in + 36);
    const int hz = trim_rsub(r, a, b);
    trim_store(out_new, r.x); trim_store(out_new + 9, r.y); trim_store(out_new + 18, r.z);
    fe t;
    fe_neg(t, r.x, 1); fe_to_b32(out_cmp, t);                                   // r.x holds -X3
    fe_to_b32(out_cmp + 32, r.y); fe_to_b32(out_cmp + 64, r.z);
    s = a; fe_neg(s.y, a.y, 1);
    fe_normalize(s.x); fe_normalize(s.y); fe_normalize(s.z);
    ge bn = b; fe_normalize(bn.x);                                              // (b.y may stay at magnitude 2: the shared form takes it)
    const int hz2 = gej_add_ge_lean(s, s, bn);
    fe_to_b32(out_cmp + 96, s.x); fe_to_b32(out_cmp + 128, s.y); fe_to_b32(out_cmp + 160, s.z);
    return hz | (hz2 << 1);
}
// in: 54 words (x = -X1, y = -Y1, zz, zzz, then the operand's x, y).  out_cmp: 8 x 32 bytes (X3, Y3, ZZ3, ZZZ3) twice.
void emu_trim_gez(u32* out_new, unsigned char* out_cmp, const u32* in) {
    gez a, s; ge b; trim_load(a.x, in); trim_load(a.y, in + 9); trim_load(a.zz, in + 18); trim_load(a.zzz, in + 27); a.inf = 0; trim_load(b.x, in + 36); trim_load(b.y, in + 45);
    s = a; fe_neg(s.x, a.x, 2); fe_neg(s.y, a.y, 1);
    fe_normalize(s.x); fe_normalize(s.y); fe_normalize(s.zz); fe_normalize(s.zzz);
    trim_gez(a, b);
    trim_store(out_new, a.x); trim_store(out_new + 9, a.y); trim_store(out_new + 18, a.zz); trim_store(out_new + 27, a.zzz);
    fe t;
    fe_neg(t, a.x, 2); fe_to_b32(out_cmp, t);
    fe_neg(t, a.y, 1); fe_to_b32(out_cmp + 32, t);
    fe_to_b32(out_cmp + 64, a.zz); fe_to_b32(out_cmp + 96, a.zzz);
    ge bn = b; fe_normalize(bn.x);
    gez_add_ge_lean(s, bn);
    fe_to_b32(out_cmp + 128, s.x); fe_to_b32(out_cmp + 160, s.y); fe_to_b32(out_cmp + 192, s.zz); fe_to_b32(out_cmp + 224, s.zzz);
}
// the chain as rp_rings_shared runs it with the signed doubling: out = 2^43 C and 2^86 C (64 bytes each), from 43 + 43 times T <- -2T
int emu_trim_chain(unsigned char* t1_64, unsigned char* t2_64, const unsigned char* c64) {
    ge a; ge_from_b64(a, c64); fe_norm_weak(a.x); fe_norm_weak(a.y);
    gej T, T1; gej_set_ge(T, a);
    for (int k = 0; k < 43; k++) gej_dblneg_ring<false>(T, T);
    T1 = T; fe_neg(T1.y, T.y, 1);
    for (int k = 0; k < 43; k++) gej_dblneg_ring<false>(T, T);
    return gej_to_b64(t1_64, T1) | gej_to_b64(t2_64, T);
}
// a step on the table of three independent bases with the point returned as fractions: returns what the step returns (0 = handed back,
// nothing produced); the digit area is a heap vector of exactly S2K_RING_DIG_WORDS words
int emu_trim_step_bases(unsigned char* r64, const unsigned char* c64, const unsigned char* t1_64, const unsigned char* t2_64,
                        const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int park_words) {
    gej A, T1, T2, R; r3p_bases(A, T1, T2, c64, t1_64, t2_64);
    scalar e, sg, f; sc_set_b32(e, e32, nullptr); sc_set_b32(sg, s32, nullptr); sc_set_b32(f, f32, nullptr);
    std::vector<u32> rtab(S2K_RTAB_WORDS, 0), rraw((size_t)park_words, 0), dig(S2K_RING_DIG_WORDS, 0);
    ecmult_ring6_tables(rtab.data(), rraw.data(), A, T1, T2);
    const int done = ecmult_ring6_step_frac(R, rtab.data(), e, sg, f, 1, gtab_host(), gtab_host(), dig.data());
    memset(r64, 0, 64);
    if (done) {
        static_assert(S2K_RING6_FRAC, "the fractions need the XYZZ table part");
        fe zi; fe_inv(zi, R.z);
        ge r; fe_mul2(r.x, R.x, zi, r.y, R.y, zi);
        fe_to_b32(r64, r.x); fe_to_b32(r64 + 32, r.y);
    }
    return done;
}
// the same on C alone (T1, T2 by the signed chain)
int emu_trim_step(unsigned char* r64, const unsigned char* c64, const unsigned char* e32, const unsigned char* s32, const unsigned char* f32, int park_words) {
    unsigned char t1[64], t2[64];
    if (emu_trim_chain(t1, t2, c64)) return -1;
    return emu_trim_step_bases(r64, c64, t1, t2, e32, s32, f32, park_words);
}
}
