// adaptor.h -- ECDSA adaptor-signature verification, one item per lane.
//   verify (secp256k1_ecdsa_adaptor_verify, src/modules/ecdsa_adaptor/main_impl.h:236-282; secp256k1_ecdsa_adaptor_sig_deserialize :31-67;
//           secp256k1_dleq_verify and secp256k1_dleq_challenge, src/modules/ecdsa_adaptor/dleq_impl.h:131-162, :62-76):
//       the 162 bytes are  R (33) | R' (33) | s' (32) | e (32) | s (32);  Y is the encryption key, X the signer's key, m the message
//       accept  <=>  everything parses (R, R' compressed points, sigr = x(R) mod n != 0, s' in [1, n), s < n; e is reduced),
//                    R1 = s*G - e*R' and R2 = s*Y - e*R are finite and H_DLEQ(R' | Y | R | R1 | R2) mod n == e      (the DLEQ half),
//                    D = (sigr/s')*X + (m/s')*G is finite and D == R' as a point                                      (the ECDSA half)
// Only this public-data call of the module is served: encrypt, decrypt and recover work on secrets and stay with the reference.
// R1 and D are ecmult_lane; R2 is the joint form ecmult_lane2 (ecmult.h), falling back to two ecmult_lane calls and a gej_add_var when it
// declines.  Flag-and-select style as ecdsa.h: an `ok` flag, the scalars of dead items zeroed, no early return in front of a
// multiplication or of the wave-shared inversion.  The lane holds no point across a multiplication: R1 (and the first product of the
// fallback) wait in `park`, and what the later stages need of the inputs is read and parsed again from global memory.
#pragma once
#include "ecdsa.h"        // ecdsa_pubkey_load, ecdsa_sc_inverse, fe_inv_lanes (waveinv.h)
#include "sha256.h"

// 1: R2 through ecmult_lane2; 0: always the two-call form (the A/B switch of tools/ab_probe.py; ecmult_lane2 stays available either way)
#ifndef S2K_ADAPTOR_JOINT
#define S2K_ADAPTOR_JOINT 1
#endif

// per-lane parking area, in words `stride` apart: R1 | the fallback's first product | y(R')
#define S2K_ADAPTOR_PARK_R1 0
#define S2K_ADAPTOR_PARK_FB S2K_PARK_GEJ_WORDS
#define S2K_ADAPTOR_PARK_RY (2 * S2K_PARK_GEJ_WORDS)
#define S2K_ADAPTOR_PARK_WORDS (2 * S2K_PARK_GEJ_WORDS + 9)

struct adaptor_midstate { u32 s[8]; };   // SHA256 state after the 64-byte tag prefix SHA256("DLEQ") x 2 (dleq_impl.h:16-22 has it as constants)
S2K_HD void adaptor_tag_midstate(adaptor_midstate& m) {
    const char tag[] = "DLEQ";
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)tag, sizeof(tag) - 1);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);     // exactly one block -> compressed
    for (int i = 0; i < 8; i++) m.s[i] = g.s[i];
}

// The challenge message is five compressed points back to back: 165 bytes behind the 64 of the tag prefix, three blocks with the padding.
// A point is its prefix byte and the eight big-endian words of x (most significant first).  Byte p of the padded message, p a constant:
S2K_HD u32 adaptor_msg_byte(int p, const u32 (*xw)[8], const u32* pre) {
    if (p < 165) {
        const int k = p / 33, o = p % 33;
        return o == 0 ? (pre[k] & 0xFFu) : ((xw[k][(o - 1) >> 2] >> (24 - 8 * ((o - 1) & 3))) & 0xFFu);
    }
    return p == 165 ? 0x80u : 0u;
}
// e = SHA256(prefix | points) mod n, overflow ignored (secp256k1_dleq_challenge)
S2K_HD void adaptor_challenge(scalar& e, const adaptor_midstate& mid, const u32 (*xw)[8], const u32* pre) {
    u32 s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = mid.s[i];
#pragma unroll
    for (int blk = 0; blk < 3; blk++) {
        u32 w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int p = 64 * blk + 4 * j;
            w[j] = (adaptor_msg_byte(p, xw, pre) << 24) | (adaptor_msg_byte(p + 1, xw, pre) << 16) | (adaptor_msg_byte(p + 2, xw, pre) << 8) | adaptor_msg_byte(p + 3, xw, pre);
        }
        if (blk == 2) { w[14] = 0u; w[15] = 8u * (64u + 165u); }       // the length in bits, tag prefix included
        sha256_compress(s, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) e.d[i] = s[7 - i];
    sc_reduce_once(e.d, sc_check_overflow(e.d));
}
// prefix and x words of a point given as 33 serialised bytes that have parsed (what secp256k1_eckey_pubkey_serialize33 would write again)
S2K_HD void adaptor_words_b33(u32 xw[8], u32& pre, const unsigned char* b33) {
    pre = b33[0];
#pragma unroll
    for (int j = 0; j < 8; j++) xw[j] = s2k_load_be32(b33 + 1 + 4 * j);
}
// ... of a normalised affine point
S2K_HD void adaptor_words_ge(u32 xw[8], u32& pre, const ge& a) {
    u32 w[8]; fe_to_words(w, a.x);
#pragma unroll
    for (int j = 0; j < 8; j++) xw[j] = w[7 - j];
    pre = 2u + (u32)fe_is_odd(a.y);
}
// ... of a public key in one of the three formats (no root is taken: a compressed key is its own serialisation)
S2K_HD void adaptor_words_key(u32 xw[8], u32& pre, const unsigned char* pk, int pk_format) {
    if (pk_format == ECDSA_PK_COMPRESSED) { adaptor_words_b33(xw, pre, pk); return; }
    ge P; ecdsa_pubkey_load(P, pk, pk_format);
    fe_normalize(P.x); fe_normalize(P.y);
    adaptor_words_ge(xw, pre, P);
}

// Returns 1 iff secp256k1_ecdsa_adaptor_verify would, for item `item` of the four arrays.  pk_format (ECDSA_PK_*) holds for pubkeys and
// enckeys alike; a key that is refused, the all-zero object included, gives 0.  park: the launch's parking area, S2K_ADAPTOR_PARK_WORDS
// words per lane, word k of lane `lane` at park[k * park_stride + lane].  The to-affine inversion is fe_inv_lanes: one per wavefront on
// the device, so EVERY lane of the wavefront must come through here.  Every stage forms its input addresses again from the array bases
// and the item number (through an offset the compiler cannot see through), so that no address is held in registers across a multiplication.
#define S2K_ADAPTOR_STAGE_INPUTS \
    const size_t it_ = item + s2k_opaque_zero(); \
    const unsigned char* const sig162 = sigs162 + 162 * it_; (void)sig162; \
    const unsigned char* const pubkey = pubkeys + ecdsa_pk_bytes(pk_format) * it_; (void)pubkey; \
    const unsigned char* const enckey = enckeys + ecdsa_pk_bytes(pk_format) * it_; (void)enckey; \
    const unsigned char* const msg32 = msgs32 + 32 * it_; (void)msg32; \
    u32* const park = park_base + (lane + s2k_opaque_zero()); (void)park
S2K_HD int adaptor_verify_lane(const adaptor_midstate& mid, const unsigned char* sigs162, const unsigned char* pubkeys, const unsigned char* msgs32,
                               const unsigned char* enckeys, size_t item, int pk_format, int live, const u32* gtab, const lane_mem& lm, u32* park_base,
                               size_t lane, size_t park_stride) {
    int ok = live;
    // ---- DLEQ half, first point: R1 = s*G - e*R'
    {
        S2K_ADAPTOR_STAGE_INPUTS;
        ge Rp; scalar en, s; int ov;
        ok &= ecdsa_pubkey_load(Rp, sig162 + 33, ECDSA_PK_COMPRESSED);
        sc_set_b32(en, sig162 + 98, nullptr); sc_negate(en, en);
        sc_set_b32(s, sig162 + 130, &ov); ok &= !ov;
#pragma unroll
        for (int i = 0; i < 9; i++) park[(S2K_ADAPTOR_PARK_RY + i) * park_stride] = Rp.y.n[i];
        if (!ok) { sc_set_zero(en); sc_set_zero(s); }
        gej Rpj, R1; gej_set_ge(Rpj, Rp);
        ecmult_lane(R1, Rpj, en, s, 1, gtab, lm);
        gej_park(park + S2K_ADAPTOR_PARK_R1 * park_stride, park_stride, R1);
    }
    // ---- second point: R2 = s*Y - e*R.  Term 0 is (Y, s), term 1 is (R, -e); the two-call form reads them again when the joint form declines
    gej R2;
    {
        int joint = 0;
        {
            S2K_ADAPTOR_STAGE_INPUTS;
            ge Rr, Y;
            ok &= ecdsa_pubkey_load(Rr, sig162, ECDSA_PK_COMPRESSED);
            ok &= ecdsa_pubkey_load(Y, enckey, pk_format);
#if S2K_ADAPTOR_JOINT
            scalar en, s;
            sc_set_b32(en, sig162 + 98, nullptr); sc_negate(en, en);
            sc_set_b32(s, sig162 + 130, nullptr);
            if (!ok) { sc_set_zero(en); sc_set_zero(s); }
            gej Yj, Rj; gej_set_ge(Yj, Y); gej_set_ge(Rj, Rr);
            joint = ecmult_lane2(R2, Yj, s, Rj, en, lm);
#endif
        }
        if (!joint) {
            S2K_ADAPTOR_STAGE_INPUTS;
            const unsigned char* const sig_again = sig162; const unsigned char* const key_again = enckey;
            auto load = [&](int k, gej& Pj, scalar& n) {
                ge P0; ecdsa_pubkey_load(P0, k ? sig_again : key_again, k ? ECDSA_PK_COMPRESSED : pk_format);
                gej_set_ge(Pj, P0);
                sc_set_b32(n, sig_again + (k ? 98 : 130), nullptr);
                if (k) sc_negate(n, n);
                if (!ok) sc_set_zero(n);
            };
            ecmult_lane2_calls(R2, load, gtab, lm, park + S2K_ADAPTOR_PARK_FB * park_stride, park_stride);
        }
    }
    // ---- both to affine with one wave-shared inversion of Z1 Z2 (a dead lane hands in 1), then the challenge
    {
        S2K_ADAPTOR_STAGE_INPUTS;
        u32 xw[5][8], pre[5];
        {
            // (only Z1 and Z2 are in registers during the inversion: X1, Y1 stay parked, X2, Y2 join them in the fallback's slot)
            u32* const p1 = park + S2K_ADAPTOR_PARK_R1 * park_stride; u32* const p2 = park + S2K_ADAPTOR_PARK_FB * park_stride;
            gej_park(p2, park_stride, R2);
            fe z1, z2, zz, one, zi, zi1, zi2;
#pragma unroll
            for (int i = 0; i < 9; i++) { z1.n[i] = p1[(18 + i) * park_stride]; z2.n[i] = p2[(18 + i) * park_stride]; }
            ok &= (!(int)p1[27 * park_stride]) & (!R2.inf);
            fe_mul(zz, z1, z2);
            ok &= !fe_normalizes_to_zero(zz);                     // (an object-format key off the curve can end at Z = 0 without the flag)
            fe_set_int(one, 1);
            fe_cmov(zz, one, !ok);
            ok &= fe_inv_lanes(zi, zz);
            fe_mul2(zi1, zi, z2, zi2, zi, z1);
            gej J; ge a;
            gej_unpark(J, p1, park_stride); ge_set_gej_zinv(a, J, zi1); adaptor_words_ge(xw[3], pre[3], a);
            gej_unpark(J, p2, park_stride); ge_set_gej_zinv(a, J, zi2); adaptor_words_ge(xw[4], pre[4], a);
        }
        adaptor_words_b33(xw[0], pre[0], sig162 + 33);
        adaptor_words_key(xw[1], pre[1], enckey, pk_format);
        adaptor_words_b33(xw[2], pre[2], sig162);
        scalar e, ee;
        adaptor_challenge(ee, mid, xw, pre);
        sc_set_b32(e, sig162 + 98, nullptr);
        ok &= sc_eq(e, ee);
    }
    // ---- ECDSA half: D = (sigr/s')*X + (m/s')*G == R'
    {
        S2K_ADAPTOR_STAGE_INPUTS;
        ge X; scalar sp, sigr, m, sn, u1, u2; int ov;
        ok &= ecdsa_pubkey_load(X, pubkey, pk_format);
        sc_set_b32(sigr, sig162 + 1, nullptr); ok &= !sc_is_zero(sigr);
        sc_set_b32(sp, sig162 + 66, &ov); ok &= (!ov) & (!sc_is_zero(sp));      // secp256k1_scalar_set_b32_seckey
        sc_set_b32(m, msg32, nullptr);
        ecdsa_sc_inverse(sn, sp);
        sc_mul(u1, sn, m); sc_mul(u2, sn, sigr);
        if (!ok) { sc_set_zero(u1); sc_set_zero(u2); }
        gej Xj, D; gej_set_ge(Xj, X);
        ecmult_lane(D, Xj, u2, u1, 1, gtab, lm);
        ok &= !D.inf;
        // D == R' without an inversion:  x(R') Z^2 == X  and  y(R') Z^3 == Y.  Both coordinates: -R' must not pass
        fe rx, ry, z2, z3, nx, ny, t0, t1;
        fe_set_b32_limit(rx, sig162 + 34);                        // (whether it is below p went into `ok` with the first stage)
#pragma unroll
        for (int i = 0; i < 9; i++) ry.n[i] = park[(S2K_ADAPTOR_PARK_RY + i) * park_stride];
        fe_sqr(z2, D.z); fe_mul(z3, z2, D.z);
        nx = D.x; fe_norm_weak(nx); fe_neg(nx, nx, 1);
        ny = D.y; fe_norm_weak(ny); fe_neg(ny, ny, 1);
        fe_mul2(t0, rx, z2, t1, ry, z3);
        fe_add(t0, nx); fe_add(t1, ny);
        ok &= fe_normalizes_to_zero(t0) & fe_normalizes_to_zero(t1);
    }
    return ok;
}
