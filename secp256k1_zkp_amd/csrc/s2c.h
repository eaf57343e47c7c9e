// s2c.h -- ECDSA sign-to-contract checks and the host's side of the anti-exfil protocol, one item per lane.
//   verify_commit (secp256k1_ecdsa_s2c_verify_commit, src/modules/ecdsa_s2c/main_impl.h:88-128; secp256k1_ec_commit, src/eccommit_impl.h:48-72):
//       accept  <=>  the opening O loads, t = H_point(ser33(O) | data32) < n, R = O + t*G is finite and x(R) mod n == r
//   host_verify   (secp256k1_anti_exfil_host_verify, :185-188):  verify_commit and secp256k1_ecdsa_verify of the same signature
//   host_commit   (secp256k1_ecdsa_anti_exfil_host_commit, :131-144):  H_data(rand32)
// H_point / H_data: SHA-256 from the state after the 64-byte prefix SHA256(tag) | SHA256(tag), tag "s2c/ecdsa/point" / "s2c/ecdsa/data"
// (the reference has both states as constants, :38-54; here they are derived on the host, as schnorr.h and adaptor.h derive theirs).
// Nothing variable is multiplied in the commitment half: t*G is tweak_gmul_fixed (tweak.h), one addition of O follows, and x(R) is
// compared with r in Jacobian coordinates as ecdsa_verify_lane compares it, so there is no inversion, no per-lane table and no digit
// stream.  Flag-and-select style as tweak.h and ecdsa.h: an `ok` flag, the tweak of a dead item zeroed, no lane returns early.
#pragma once
#include "tweak.h"

#define S2C_OPENING_COMPRESSED 0
#define S2C_OPENING_OBJECT 1

S2K_HD size_t s2c_opening_bytes(int opening_format) { return opening_format == S2C_OPENING_OBJECT ? 64 : 33; }

struct s2c_midstates { u32 point[8], data[8]; };
S2K_HD void s2c_tag_midstate(u32 out[8], const char* tag, size_t len) {
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)tag, len);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);     // exactly one block -> compressed
    for (int i = 0; i < 8; i++) out[i] = g.s[i];
}
S2K_HD void s2c_tag_midstates(s2c_midstates& m) {
    s2c_tag_midstate(m.point, "s2c/ecdsa/point", 15);
    s2c_tag_midstate(m.data, "s2c/ecdsa/data", 14);
}

// opening_format 0: 33 bytes compressed (secp256k1_ecdsa_s2c_opening_parse is secp256k1_ec_pubkey_parse); 1: the 64-byte
// secp256k1_ecdsa_s2c_opening object, which has the layout of secp256k1_pubkey (an all-zero x gives 0, as in the other calls)
S2K_HD int s2c_opening_load(ge& O, const unsigned char* opening, int opening_format) {
    return ecdsa_pubkey_load(O, opening, opening_format == S2C_OPENING_OBJECT ? ECDSA_PK_OBJECT : ECDSA_PK_COMPRESSED);
}

// t32 = H_point(ser33(O) | data32), ser33 as secp256k1_ec_commit_pubkey_serialize_const writes it (eccommit_impl.h:16-25): 02 / 03 by
// the parity of the normalised y, then x big-endian.  Behind the 64 bytes of the midstate the 33 + 32 bytes fill one block and put
// one byte into the next; both blocks are put together from words (129 bytes in all), so no byte buffer is needed.
S2K_HD void s2c_tweak(unsigned char t32[32], const s2c_midstates& mid, const ge& opening, const unsigned char* data32) {
    fe x = opening.x, y = opening.y;
    fe_normalize(x); fe_normalize(y);
    u32 xl[8], xw[8], dw[8], w[16], st[8];
    fe_to_words(xl, x);
#pragma unroll
    for (int j = 0; j < 8; j++) { xw[j] = xl[7 - j]; dw[j] = s2k_load_be32(data32 + 4 * j); st[j] = mid.point[j]; }
    w[0] = ((u32)(2 + fe_is_odd(y)) << 24) | (xw[0] >> 8);
#pragma unroll
    for (int j = 1; j < 8; j++) w[j] = (xw[j - 1] << 24) | (xw[j] >> 8);
    w[8] = (xw[7] << 24) | (dw[0] >> 8);
#pragma unroll
    for (int j = 1; j < 8; j++) w[8 + j] = (dw[j - 1] << 24) | (dw[j] >> 8);
    sha256_compress(st, w);
    w[0] = (dw[7] << 24) | 0x00800000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 8u * 129u;
    sha256_compress(st, w);
#pragma unroll
    for (int j = 0; j < 8; j++) s2k_store_be32(t32 + 4 * j, st[j]);
}

// x(R) mod n == r, R finite: the comparison of ecdsa_verify_lane (ecdsa_impl.h:241-270),  r Z^2 == X,  or  r < p - n  and
// (r + n) Z^2 == X.  This is secp256k1_scalar_set_b32(&x_scalar, x_bytes, NULL) followed by secp256k1_scalar_eq (main_impl.h:116-127)
// without the to-affine inversion secp256k1_ec_commit pays.  r < n.
S2K_HD int s2c_x_matches(const gej& R, const scalar& r) {
    fe xr, xn, z2, nx, t0, t1;
    fe_from_words(xr, r.d);                                       // r < n < p: canonical
    ecdsa_fe_order(xn); fe_add(xn, xr);                           // magnitude 2
    fe_sqr(z2, R.z);
    nx = R.x; fe_norm_weak(nx); fe_neg(nx, nx, 1);                // magnitude 2
    fe_mul2(t0, xr, z2, t1, xn, z2);
    fe_add(t0, nx); fe_add(t1, nx);                               // magnitude 3
    return fe_normalizes_to_zero(t0) | (ecdsa_below_p_minus_n(r) & fe_normalizes_to_zero(t1));
}

// The commitment half behind the signature parser: 1 iff ok, the opening loads, t < n, R = O + t*G is finite and x(R) mod n == r.
// The sum is tweak_sum_lane's (t == 0: R = O; t*G == O: the doubling; t*G == -O: infinity) with the opening held across the window
// loop: it was lifted for the hash, and tweak_sum_lane, which takes the key as bytes, would take its square root a second time.
S2K_HD int s2c_commit_core(const scalar& r, int ok, const s2c_midstates& mid, const unsigned char* data32, const unsigned char* opening, int opening_format,
                           const u32* gtab) {
    ge O; int ov;
    ok &= s2c_opening_load(O, opening, opening_format);
    unsigned char t32[32];
    s2c_tweak(t32, mid, O, data32);
    scalar t;
    sc_set_b32(t, t32, &ov); ok &= !ov;                          // t >= n: secp256k1_ec_commit_tweak_add fails (secp256k1_eckey_pubkey_tweak_add)
    if (!ok) sc_set_zero(t);
    gej T, R; tweak_gmul_fixed(T, gtab, t.d);
    const int f = gej_add_ge(R, T, O);
    if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, R); R = d; }
    ok &= !R.inf;
    ok &= s2c_x_matches(R, r);
    return ok;
}

// Returns 1 iff secp256k1_ecdsa_s2c_verify_commit would on what the parsers make of these bytes.  Only r is used: s is not examined
// beyond what the signature parser refuses.  `size` is only read for DER.
S2K_HD int s2c_commit_lane(const s2c_midstates& mid, const unsigned char* sig, u64 size, int sig_format, const unsigned char* data32, const unsigned char* opening,
                           int opening_format, int live, const u32* gtab) {
    scalar r, s;
    const int ok = live & ecdsa_sig_load(r, s, sig, size, sig_format);
    return s2c_commit_core(r, ok, mid, data32, opening, opening_format, gtab);
}

// Returns 1 iff secp256k1_anti_exfil_host_verify would: s2c_commit_lane & ecdsa_verify_lane on one parse of the signature.  The
// commitment half runs first, so that its registers are dead before ecmult_lane starts; an item it refuses walks ecmult_lane with zero
// scalars, in lock step with its wavefront.  The ECDSA half is ecdsa_verify_lane's body behind the parser (ecdsa.h).
S2K_HD int s2c_host_verify_lane(const s2c_midstates& mid, const unsigned char* sig, u64 size, int sig_format, const unsigned char* msghash32, const unsigned char* pk,
                                int pk_format, const unsigned char* host_data32, const unsigned char* opening, int opening_format, int live, const u32* gtab,
                                const lane_mem& lm) {
    scalar r, s, m, sn, u1, u2; ge P;
    int ok = live & ecdsa_sig_load(r, s, sig, size, sig_format);
    ok = s2c_commit_core(r, ok, mid, host_data32, opening, opening_format, gtab);
    ok &= ecdsa_pubkey_load(P, pk, pk_format);
    sc_set_b32(m, msghash32, nullptr);
    ok &= !sc_is_zero(r) & !sc_is_zero(s) & !sc_is_high(s);       // secp256k1_ecdsa_verify refuses s > n/2 although parsing accepts it
    ecdsa_sc_inverse(sn, s);
    sc_mul(u1, sn, m); sc_mul(u2, sn, r);
    if (!ok) { sc_set_zero(u1); sc_set_zero(u2); }
    gej Pj, R; gej_set_ge(Pj, P);
    ecmult_lane(R, Pj, u2, u1, 1, gtab, lm);
    ok &= !R.inf;
    ok &= s2c_x_matches(R, r);
    return ok;
}

// out32 = H_data(rand32): one block (32 bytes behind the 64 of the midstate)
S2K_HD void s2c_host_commit_lane(unsigned char* out32, const s2c_midstates& mid, const unsigned char* rand32) {
    u32 w[16], st[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = s2k_load_be32(rand32 + 4 * j); st[j] = mid.data[j]; }
    w[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; j++) w[j] = 0;
    w[15] = 8u * 96u;
    sha256_compress(st, w);
#pragma unroll
    for (int j = 0; j < 8; j++) s2k_store_be32(out32 + 4 * j, st[j]);
}
