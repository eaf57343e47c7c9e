// ecdsa.h -- ECDSA verification and public-key recovery, one item per lane.
//   verify  (secp256k1_ecdsa_verify, src/secp256k1.c:498-512; secp256k1_ecdsa_sig_verify, src/ecdsa_impl.h:195-272):
//       accept  <=>  r, s != 0, s <= n/2, R = (r/s)*P + (m/s)*G is finite and x(R) == r (mod n)
//   recover (secp256k1_ecdsa_recover, src/modules/recovery/main_impl.h:87-157):
//       Q = (s/r)*X + (-m/r)*G with X the point lifted from r (+ n when recid & 2), parity recid & 1
// plus the parsers in front of them: compact / object / DER signatures (secp256k1_ecdsa_sig_parse, ecdsa_impl.h:141-193) and
// compressed / object / uncompressed-or-hybrid public keys (secp256k1_eckey_pubkey_parse, src/eckey_impl.h:18-36).
// The double multiplication is ecmult_lane (ecmult.h).  Flag-and-select style as schnorr.h: an `ok` flag, the scalars of dead items
// zeroed, no early return in front of ecmult_lane, so a wavefront walks it in lock step.
#pragma once
#include "ecmult.h"
#include "schnorr.h"      // fe_set_le32
#include "waveinv.h"

#define ECDSA_SIG_COMPACT 0
#define ECDSA_SIG_OBJECT 1
#define ECDSA_SIG_DER 2
#define ECDSA_PK_COMPRESSED 0
#define ECDSA_PK_OBJECT 1
#define ECDSA_PK_FULL 2

S2K_HD size_t ecdsa_pk_bytes(int pk_format) { return pk_format == ECDSA_PK_COMPRESSED ? 33 : pk_format == ECDSA_PK_OBJECT ? 64 : 65; }

// 1/s mod n.  Per lane: variable-time division steps (sc_inverse), so the lanes of a wavefront diverge inside it; its measured share of
// k_ecdsa_verify is in DESIGN.md 7.1.  -DS2K_ECDSA_DIAG_NO_SCINV (diagnostic builds only; verdicts are meaningless then) replaces it
// by a copy: the difference of the two kernel times is that share (tools/ecdsa_parts.py).
S2K_HD void ecdsa_sc_inverse(scalar& r, const scalar& a) {
#if defined(S2K_ECDSA_DIAG_NO_SCINV)
    r = a;
#else
    sc_inverse(r, a);
#endif
}

// ---- DER (ecdsa_impl.h:36-169).  Positions are offsets into sig[0 .. end); lengths are 64-bit as the reference's size_t. ------------
S2K_HD int ecdsa_der_read_len(u64& len, const unsigned char* sig, u64& pos, u64 end) {
    len = 0;
    if (pos >= end) return 0;
    const u32 b1 = sig[pos++];
    if (b1 == 0xFF) return 0;                                   // X.690 8.1.3.5.c
    if ((b1 & 0x80) == 0) { len = b1; return 1; }               // short form
    if (b1 == 0x80) return 0;                                   // indefinite length
    u64 lenleft = b1 & 0x7F;
    if (lenleft > end - pos) return 0;
    if (sig[pos] == 0) return 0;                                // not the shortest length encoding
    if (lenleft > 8) return 0;                                  // would exceed a size_t
    while (lenleft > 0) { len = (len << 8) | sig[pos]; pos++; lenleft--; }
    if (len > end - pos) return 0;
    if (len < 128) return 0;                                    // not the shortest length encoding
    return 1;
}
// an integer that is negative, longer than 32 bytes or >= n parses as 0 (and the signature then fails on r == 0 / s == 0)
S2K_HD int ecdsa_der_parse_integer(scalar& r, const unsigned char* sig, u64& pos, u64 end) {
    int overflow = 0;
    u64 rlen;
    sc_set_zero(r);
    if (pos == end || sig[pos] != 0x02) return 0;
    pos++;
    if (!ecdsa_der_read_len(rlen, sig, pos, end)) return 0;
    if (rlen == 0 || rlen > end - pos) return 0;
    if (sig[pos] == 0x00 && rlen > 1 && (sig[pos + 1] & 0x80) == 0x00) return 0;      // excessive 0x00 padding
    if (sig[pos] == 0xFF && rlen > 1 && (sig[pos + 1] & 0x80) == 0x80) return 0;      // excessive 0xFF padding
    if (sig[pos] & 0x80) overflow = 1;                                                // negative
    if (sig[pos] == 0) { rlen--; pos++; }                                             // the one leading zero byte
    if (rlen > 32) overflow = 1;
    const unsigned char* last = sig + pos + rlen;                                     // byte k from the least significant end is last[-1 - k]
    const u32 take = overflow ? 0u : (u32)rlen;
#pragma unroll
    for (int j = 0; j < 8; j++) {                                                     // (constant limb indices: nothing goes to scratch)
        u32 w = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) if ((u32)(4 * j + b) < take) w |= (u32)last[-1 - (4 * j + b)] << (8 * b);
        r.d[j] = w;
    }
    overflow |= sc_check_overflow(r.d);
    if (overflow) sc_set_zero(r);
    pos += rlen;
    return 1;
}
S2K_HD int ecdsa_der_parse(scalar& r, scalar& s, const unsigned char* sig, u64 size) {
    u64 pos = 0, rlen;
    sc_set_zero(r); sc_set_zero(s);
    if (size == 0 || sig[pos++] != 0x30) return 0;
    if (!ecdsa_der_read_len(rlen, sig, pos, size)) return 0;
    if (rlen != size - pos) return 0;                           // tuple exceeds bounds or garbage after it
    if (!ecdsa_der_parse_integer(r, sig, pos, size)) return 0;
    if (!ecdsa_der_parse_integer(s, sig, pos, size)) return 0;
    return pos == size;                                         // trailing garbage inside the tuple
}

// sig_format 0: 64 bytes r | s big-endian (secp256k1_ecdsa_signature_parse_compact: r or s >= n fails); 1: the 64-byte
// secp256k1_ecdsa_signature object, the little-endian limbs of r then s (secp256k1.c:393-405; limbs >= n, which no parser
// produces, give 0); 2: DER, `size` bytes.
S2K_HD int ecdsa_sig_load(scalar& r, scalar& s, const unsigned char* sig, u64 size, int sig_format) {
    int ok = 1;
    if (sig_format == ECDSA_SIG_DER) {
        ok = ecdsa_der_parse(r, s, sig, size);
    } else if (sig_format == ECDSA_SIG_OBJECT) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            r.d[i] = (u32)sig[4 * i] | ((u32)sig[4 * i + 1] << 8) | ((u32)sig[4 * i + 2] << 16) | ((u32)sig[4 * i + 3] << 24);
            s.d[i] = (u32)sig[32 + 4 * i] | ((u32)sig[32 + 4 * i + 1] << 8) | ((u32)sig[32 + 4 * i + 2] << 16) | ((u32)sig[32 + 4 * i + 3] << 24);
        }
        ok = !sc_check_overflow(r.d) & !sc_check_overflow(s.d);
    } else {
        int ov;
        sc_set_b32(r, sig, &ov); ok &= !ov;
        sc_set_b32(s, sig + 32, &ov); ok &= !ov;
    }
    if (!ok) { sc_set_zero(r); sc_set_zero(s); }
    return ok;
}

// pk_format 0: 33 bytes compressed; 1: the 64-byte secp256k1_pubkey object (x, y as 32 little-endian bytes each; x == 0, where the
// reference raises its illegal-argument callback, gives 0); 2: 65 bytes uncompressed (04) or hybrid (06 / 07).
// P always comes back with magnitude-1 coordinates, also when the key is refused.
S2K_HD int ecdsa_pubkey_load(ge& P, const unsigned char* pk, int pk_format) {
    int ok = 1;
    if (pk_format == ECDSA_PK_OBJECT) {
        fe_set_le32(P.x, pk); fe_set_le32(P.y, pk + 32);
        fe_normalize(P.x); fe_normalize(P.y);
        ok &= !fe_is_zero_normalized(P.x);
    } else if (pk_format == ECDSA_PK_COMPRESSED) {
        fe x;
        ok &= (pk[0] == 0x02) | (pk[0] == 0x03);
        ok &= fe_set_b32_limit(x, pk + 1);
        ok &= ge_set_xo(P, x, pk[0] == 0x03);
        fe_norm_weak(P.y);
    } else {
        const int hybrid = (pk[0] == 0x06) | (pk[0] == 0x07);
        ok &= (pk[0] == 0x04) | hybrid;
        ok &= fe_set_b32_limit(P.x, pk + 1);
        ok &= fe_set_b32_limit(P.y, pk + 33);
        ok &= !hybrid | (fe_is_odd(P.y) == (pk[0] == 0x07));      // (y < p whenever ok is still set: its limbs are canonical)
        ok &= ge_is_valid(P);
    }
    return ok;
}

// a < p - n = 0x1 45512319 50B75FC4 402DA172 2FC9BAEE ?  (secp256k1_ecdsa_const_p_minus_order)
S2K_HD int ecdsa_below_p_minus_n(const scalar& a) {
    const u32 c[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u, 1u, 0u, 0u, 0u};
    int lt = 0, gt = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt |= (a.d[i] < c[i]) & ~gt;
        gt |= (a.d[i] > c[i]) & ~lt;
    }
    return lt;
}
S2K_HD void ecdsa_fe_order(fe& r) {
    const u32 w[8] = {SC_N0, SC_N1, SC_N2, SC_N3, SC_N4, SC_N5, SC_N6, SC_N7};
    fe_from_words(r, w);
}

// Returns 1 iff the signature verifies.  `size` is only read for DER.
S2K_HD int ecdsa_verify_lane(const unsigned char* sig, u64 size, int sig_format, const unsigned char* msghash32, const unsigned char* pk, int pk_format,
                             int live, const u32* gtab, const lane_mem& lm) {
    int ok = live;
    scalar r, s, m, sn, u1, u2; ge P;
    ok &= ecdsa_sig_load(r, s, sig, size, sig_format);
    ok &= ecdsa_pubkey_load(P, pk, pk_format);
    sc_set_b32(m, msghash32, nullptr);
    ok &= !sc_is_zero(r) & !sc_is_zero(s) & !sc_is_high(s);       // secp256k1_ecdsa_verify refuses s > n/2 although parsing accepts it
    ecdsa_sc_inverse(sn, s);
    sc_mul(u1, sn, m); sc_mul(u2, sn, r);
    if (!ok) { sc_set_zero(u1); sc_set_zero(u2); }
    gej Pj, R; gej_set_ge(Pj, P);
    ecmult_lane(R, Pj, u2, u1, 1, gtab, lm);
    ok &= !R.inf;
    // x(R) == r (mod n) without an inversion (ecdsa_impl.h:241-270):  xr Z^2 == X,  or  xr < p - n  and  (xr + n) Z^2 == X
    fe xr, xn, z2, nx, t0, t1;
    fe_from_words(xr, r.d);                                       // r < n < p: canonical
    ecdsa_fe_order(xn); fe_add(xn, xr);                           // magnitude 2
    fe_sqr(z2, R.z);
    nx = R.x; fe_norm_weak(nx); fe_neg(nx, nx, 1);                // magnitude 2
    fe_mul2(t0, xr, z2, t1, xn, z2);
    fe_add(t0, nx); fe_add(t1, nx);                               // magnitude 3
    ok &= fe_normalizes_to_zero(t0) | (ecdsa_below_p_minus_n(r) & fe_normalizes_to_zero(t1));
    return ok;
}

// fe (normalised) -> 32 little-endian bytes: one half of a secp256k1_pubkey object
S2K_HD void ecdsa_fe_get_le32(unsigned char* b, const fe& a) {
    u32 w[8]; fe_to_words(w, a);
#pragma unroll
    for (int j = 0; j < 8; j++) { b[4 * j] = (unsigned char)w[j]; b[4 * j + 1] = (unsigned char)(w[j] >> 8); b[4 * j + 2] = (unsigned char)(w[j] >> 16); b[4 * j + 3] = (unsigned char)(w[j] >> 24); }
}

// Returns 1 and the recovered key as a 64-byte secp256k1_pubkey object (what pk_format 1 reads), or 0 and 64 zero bytes.  sig64 is
// compact r | s; recid other than 0..3 gives 0.  Nothing is written when !live.  The to-affine inversion is fe_inv_lanes: one per
// wavefront on the device, so EVERY lane of the wavefront must come through here, and a lane without a finite result hands in z = 1.
S2K_HD int ecdsa_recover_lane(unsigned char* pubkey_out64, const unsigned char* sig64, unsigned recid, const unsigned char* msghash32,
                              int live, const u32* gtab, const lane_mem& lm) {
    int ok = live, ov;
    scalar r, s, m, rn, u1, u2; ge X;
    sc_set_b32(r, sig64, &ov); ok &= !ov;
    sc_set_b32(s, sig64 + 32, &ov); ok &= !ov;
    sc_set_b32(m, msghash32, nullptr);
    ok &= recid <= 3u;
    ok &= !sc_is_zero(r) & !sc_is_zero(s);
    fe fx, fxn;
    fe_from_words(fx, r.d);
    ecdsa_fe_order(fxn); fe_add(fxn, fx);
    const int plus_n = (recid & 2u) != 0;
    ok &= !plus_n | ecdsa_below_p_minus_n(r);                     // r + n must stay below p
    fe_cmov(fx, fxn, plus_n);
    fe_normalize(fx);
    ok &= ge_set_xo(X, fx, (int)(recid & 1u));
    fe_norm_weak(X.y);
    ecdsa_sc_inverse(rn, r);
    sc_mul(u1, rn, m); sc_negate(u1, u1);
    sc_mul(u2, rn, s);
    if (!ok) { sc_set_zero(u1); sc_set_zero(u2); }
    gej Xj, Q; gej_set_ge(Xj, X);
    ecmult_lane(Q, Xj, u2, u1, 1, gtab, lm);
    ok &= !Q.inf;
    fe z = Q.z, one, zi, zi2, zi3; ge a;
    fe_set_int(one, 1);
    fe_cmov(z, one, !ok);
    ok &= fe_inv_lanes(zi, z);                                   // 0: some lane of the wavefront handed in z == 0, every inverse is meaningless
    fe_sqr(zi2, zi); fe_mul(zi3, zi2, zi);
    fe_mul2(a.x, Q.x, zi2, a.y, Q.y, zi3);
    fe_normalize(a.x); fe_normalize(a.y);
    if (live) {
        if (ok) { ecdsa_fe_get_le32(pubkey_out64, a.x); ecdsa_fe_get_le32(pubkey_out64 + 32, a.y); }
        else for (int i = 0; i < 64; i++) pubkey_out64[i] = 0;
    }
    return ok;
}
