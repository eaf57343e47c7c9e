// ellswift.h -- BIP-324's ElligatorSwift encoding of public keys, the two calls that read public data only, one item per lane.
//   decode (secp256k1_ellswift_decode, src/modules/ellswift/main_impl.h:470-483, over secp256k1_ellswift_xswiftec_frac_var :24-132):
//       64 bytes u | t  ->  the point whose x is the first of x3, x2, x1 on the curve and whose y has the parity of t.  Every input decodes.
//   encode (secp256k1_ellswift_encode :393-420, over secp256k1_ellswift_xelligatorswift_var :333-367 and xswiftec_inv_var :168-303):
//       a public key and 32 bytes of public randomness -> 64 bytes, by a rejection loop over hash-derived (u, branch) pairs.
// secp256k1_ellswift_create and secp256k1_ellswift_xdh handle a secret key and stay with the reference.
// Square tests: csrc/ has no Jacobi symbol, so fe_sqrt is the square test (as in generator.h).  A candidate n / d is on the curve iff
// m = (n^3 + 7 d^3) d is a square, and m = d^4 (x^3 + 7), so the root that tests the chosen candidate is also d^2 y: decode to a full
// key costs at most three roots and ONE inversion (x = n / d, y = +-root / d^2), decode to x only two roots (x1 needs no test) and the
// inversion.  The inversion is fe_inv_lanes (waveinv.h), one per wavefront: no lane may leave in front of it, and a lane without an
// item, or a dead one, hands in 1.  Flag-and-select style as tweak.h, generator.h and s2c.h.
// The one deviation from the reference: the encode loop is bounded (ELLSWIFT_MAX_ATTEMPTS); see ellswift_encode_lane.
#pragma once
#include "tweak.h"        // tweak_key_load, ecdsa_fe_get_le32; ecdsa.h -> ecmult.h (S2K_WAVE_ANY), waveinv.h
#include "sha256.h"

#define ELLSWIFT_OUT_X 0
#define ELLSWIFT_OUT_OBJECT 1
#define ELLSWIFT_OUT_COMPRESSED 2
// Four pools of 64 branch values.  An attempt succeeds with probability about 1/4, so an item gets here with probability
// (3/4)^256 ~ 1e-32; the reference loops until it succeeds, a kernel on a shared machine may not.
#define ELLSWIFT_MAX_ATTEMPTS 256u

S2K_HD size_t ellswift_out_bytes(int out_format) { return out_format == ELLSWIFT_OUT_X ? 32 : out_format == ELLSWIFT_OUT_OBJECT ? 64 : 33; }

// c1 = (sqrt(-3) - 1) / 2 (main_impl.h:14-21); c2 = -c1 - 1, c3 = -c1, c4 = c1 + 1 follow from it.  All come back with magnitude 1.
S2K_HD void ellswift_fe_c1(fe& r) {
    const u32 w[8] = {0x8e6afa40u, 0x3ec693d6u, 0xed0a766au, 0x630fb68au, 0x53cbcb16u, 0x919bb861u, 0x9a83f8efu, 0x851695d4u};
    fe_from_words(r, w);
}
S2K_HD void ellswift_fe_c4(fe& r) { ellswift_fe_c1(r); r.n[0] += 1u; }                                 // (limb 0 of c1 is even: no carry)
S2K_HD void ellswift_fe_c3(fe& r) { fe c; ellswift_fe_c1(c); fe_neg(r, c, 1); fe_norm_weak(r); }
S2K_HD void ellswift_fe_c2(fe& r) { fe c; ellswift_fe_c4(c); fe_neg(r, c, 1); fe_norm_weak(r); }

// (n^3 + 7 d^3) d: a square iff n / d is the x of a point (secp256k1_ge_x_frac_on_curve_var).  n, d magnitude 1; r magnitude 1.
S2K_HD void ellswift_frac_rhs(fe& r, const fe& n, const fe& d) {
    fe n2, d2, n3, d3;
    fe_sqr2(n2, n, d2, d);
    fe_mul2(n3, n2, n, d3, d2, d);
    fe_mul_int(d3, 7); fe_norm_weak(d3);
    fe_add(n3, d3);                                               // magnitude 2
    fe_mul(r, n3, d);
}

// secp256k1_ellswift_xswiftec_frac_var with the root kept: u = 0 -> 1, t = 0 -> s = 1, g + s = 0 -> s <- 4 s, then the first of
// x3 = (3 s u^3 - (g + s)^2) / (3 s u^2), x2 = u (c1 s + c2 g) / (g + s), x1 = -(x2 + u) that is on the curve.  u is any 32-byte value
// (fe_set_b32_mod: u >= p is legal and is reduced by the arithmetic), t is NORMALISED (its zero test and, in the caller, its parity
// are those of the reduced value).  roots = 3: every candidate is tested, `root` is the root of (n^3 + 7 d^3) d of the one taken;
// roots = 2: x1 is taken untested when x3 and x2 fail, `root` is then meaningless.  Returns which candidate was taken: 3, 2 or 1.
// The denominators are never 0: u != 0 and s != 0 after the substitutions (t != 0 gives t^2 != 0), so 3 s u^2 != 0; and when
// g + s = 0 the new sum is g + 4 s = 3 s != 0.  xn, xd: magnitude 1.
S2K_HD int ellswift_frac_root(fe& xn, fe& xd, fe& root, const fe& u_in, const fe& t, int roots) {
    fe u = u_in, one, s, l, g, p, d, n3, n2, n1;
    fe_set_int(one, 1);
    fe_cmov(u, one, fe_normalizes_to_zero(u));
    fe_sqr(s, t); fe_cmov(s, one, fe_is_zero_normalized(t));
    fe_sqr(l, u); fe_mul(g, l, u); g.n[0] += 7u; fe_norm_weak(g);                  // g = u^3 + 7
    fe_add2(p, g, s);
    {
        const int z = fe_normalizes_to_zero(p);
        fe s4 = s; fe_mul_int(s4, 4); fe_norm_weak(s4);
        fe_cmov(s, s4, z);
    }
    fe_add2(p, g, s); fe_norm_weak(p);                                             // p = g + s
    fe_mul(d, s, l); fe_mul_int(d, 3); fe_norm_weak(d);                            // d = 3 s u^2
    {
        fe p2, c1, c2, a, b, up;
        fe_mul_sqr(n3, d, u, p2, p);
        fe_neg(p2, p2, 1); fe_add(n3, p2); fe_norm_weak(n3);                       // n3 = 3 s u^3 - (g + s)^2
        ellswift_fe_c1(c1); ellswift_fe_c2(c2);
        fe_mul2(a, c1, s, b, c2, g); fe_add(a, b);                                 // c1 s + c2 g, magnitude 2
        fe_mul2(n2, a, u, up, p, u);                                               // n2 = u (c1 s + c2 g)
        fe_add2(n1, n2, up); fe_neg(n1, n1, 2); fe_norm_weak(n1);                  // n1 = -(n2 + u (g + s))
    }
    int found = 0, which = 0;
    fe_set_zero(xn); fe_set_zero(xd); fe_set_zero(root);
#pragma unroll 1
    for (int k = 0; k < 3; k++) {                                                  // rolled: one fe_sqrt body
        fe n = n3, dd = p, m, r;
        fe_cmov(n, n2, k == 1); fe_cmov(n, n1, k == 2);
        fe_cmov(dd, d, k == 0);
        int q = 1;
        fe_set_zero(r);
        if (k < roots) { ellswift_frac_rhs(m, n, dd); q = fe_sqrt(r, m); }
        const int take = (!found) & (q | (k == 2));                                 // (x1 is on the curve whenever x3 and x2 are not)
        fe_cmov(xn, n, take); fe_cmov(xd, dd, take); fe_cmov(root, r, take);
        which = take ? 3 - k : which;
        found |= take;
    }
    return which;
}
S2K_HD int ellswift_xswiftec_frac(fe& xn, fe& xd, const fe& u, const fe& t) {
    fe root;
    return ellswift_frac_root(xn, xd, root, u, t, 2);
}

// secp256k1_ellswift_decode for one item.  out_format 0: ser32(x) (secp256k1_ellswift_xswiftec_var: no root for y is taken); 1: the
// 64-byte secp256k1_pubkey object; 2: 33 bytes compressed.  The wave-shared inversion is in here: EVERY lane of the wavefront comes
// through, a lane without an item hands in 1.  Nothing is written when !live.
S2K_HD void ellswift_decode_lane(unsigned char* out, int out_format, const unsigned char* ell64, int live) {
    fe u, t, xn, xd, root, one, di, x;
    fe_set_b32_mod(u, ell64); fe_set_b32_mod(t, ell64 + 32);
    fe_normalize(t);
    ellswift_frac_root(xn, xd, root, u, t, out_format == ELLSWIFT_OUT_X ? 2 : 3);
    fe_set_int(one, 1);
    fe_cmov(xd, one, !live);
    fe_inv_lanes(di, xd);
    fe_mul(x, xn, di); fe_normalize(x);
    if (out_format == ELLSWIFT_OUT_X) {
        if (live) fe_get_b32(out, x);
        return;
    }
    fe di2, y, ny;
    fe_sqr(di2, di); fe_mul(y, root, di2); fe_normalize(y);                        // root^2 = d^4 (x^3 + 7)
    fe_neg(ny, y, 1); fe_normalize(ny);
    fe_cmov(y, ny, fe_is_odd(y) != fe_is_odd(t));                                  // (secp256k1_ge_set_xo_var with the parity of the reduced t; y != 0 on this curve)
    if (live) {
        if (out_format == ELLSWIFT_OUT_OBJECT) { ecdsa_fe_get_le32(out, x); ecdsa_fe_get_le32(out + 32, y); }
        else { out[0] = (unsigned char)(2 + fe_is_odd(y)); fe_get_b32(out + 1, x); }
    }
}

// secp256k1_ellswift_xswiftec_inv_var for c in 0..7: 1 and t with xswiftec(u, t) = x, or 0.  x on the curve, u != 0.
// Both arms of the reference ((c & 2) = 0: an inverse under x1 / x2; (c & 2) = 2: under x3) walk the same three roots and the one
// wave-shared inversion here, so that lanes with different c stay in lock step:
//   root 1   arm 0: (-u-x)^3 + 7, refused when it IS a square (:209)          arm 1: s = x - u, refused when it is not (:256)
//   root 2   arm 0: -(u^3+7)(u^2+ux+x^2), refused when not a square (:239)     arm 1: q = -s (4 (u^3+7) + 3 u^2 s), likewise (:268); r = its root
//                                                                              arm 1: refused when c & 1 and r = 0 (:277), and when s = 0 (:280)
//   inverse  arm 0: of -(u^2+ux+x^2); s = (u^3+7) times it, v = x             arm 1: of s; v = (r / s - u) / 2
//   root 3   w = sqrt(s) (arm 1: the value root 1 already gave)
//   t = +-w (c3 u + v) or +-w (c4 u + v) by c & 5.
// `active` 0: a lane that has nothing to invert (finished, dead or without an item).  Such a lane, a refused one, and one whose
// denominator is 0 -- arm 1 with s = 0; arm 0 cannot have it for x on the curve (the reference's argument at :217-229), an object off
// the curve might -- hand 1 to the inversion, so no lane poisons its wavefront.  Every lane of the wavefront must come through.
S2K_HD int ellswift_xswiftec_inv(fe& t, const fe& x_in, const fe& u_in, int c, int active = 1) {
    fe x = x_in, u = u_in, one, u2, g, m, s0, s1, ux;
    fe_norm_weak(x); fe_norm_weak(u);
    fe_set_int(one, 1);
    const int b = (c >> 1) & 1;
    int ok = active;
    fe_sqr(u2, u); fe_mul(g, u2, u); g.n[0] += 7u; fe_norm_weak(g);               // g = u^3 + 7
    fe_add2(m, x, u); fe_neg(m, m, 2); fe_norm_weak(m);                            // m = -u - x
    fe_mul_sqr(ux, u, x, s0, m);
    fe_neg(s0, s0, 1); fe_add(s0, ux); fe_norm_weak(s0);                           // s0 = -(u^2 + u x + x^2)
    fe_neg(s1, u, 1); fe_add(s1, x); fe_norm_weak(s1);                             // s1 = x - u
    fe a, r1, r2;
    ge_curve_rhs(a, m); fe_norm_weak(a);
    fe_cmov(a, s1, b);
    const int q1 = fe_sqrt(r1, a);
    ok &= b ? q1 : !q1;
    {
        fe qb, g4 = g;
        fe_mul(qb, s1, u2); fe_mul_int(qb, 3); fe_mul_int(g4, 4); fe_add(qb, g4); fe_norm_weak(qb);       // 4 g + 3 u^2 s1 (magnitude 7 -> 1)
        fe_mul2(qb, qb, s1, a, s0, g);
        fe_neg(qb, qb, 1); fe_norm_weak(qb);
        fe_cmov(a, qb, b);
    }
    ok &= fe_sqrt(r2, a);
    ok &= !(b & (c & 1) & fe_normalizes_to_zero(r2));
    fe den = s0, di, e, s, v;
    fe_cmov(den, s1, b);
    ok &= !fe_normalizes_to_zero(den);
    fe_cmov(den, one, !ok);
    fe_inv_lanes(di, den);
    e = g; fe_cmov(e, r2, b);
    fe_mul(e, e, di);                                                              // arm 0: s = g / s0; arm 1: r / s
    s = e; fe_cmov(s, s1, b);
    v = u; fe_neg(v, v, 1); fe_add(v, e); fe_norm_weak(v); fe_half(v);             // (r / s - u) / 2
    fe_cmov(v, x, !b);
    fe w, nw, cc, c4;
    ok &= fe_sqrt(w, s);                                                           // (a square whenever ok is still set)
    fe_neg(nw, w, 1);
    fe_cmov(w, nw, ((c & 5) == 0) | ((c & 5) == 5));                               // magnitude 2
    ellswift_fe_c3(cc); ellswift_fe_c4(c4); fe_cmov(cc, c4, c & 1);
    fe_mul(cc, cc, u); fe_add(cc, v);                                              // magnitude 2
    fe_mul(t, w, cc);
    return ok;
}

// ---- the encode's generator (secp256k1_ellswift_prng :310-325 over the state secp256k1_ellswift_encode sets up :402-410) ------------
// SHA-256 from the state after the 64-byte prefix SHA256(tag) | SHA256(tag), tag "secp256k1_ellswift_encode" (the reference has it as
// constants, :385-391; here it is derived on the host, as s2c_tag_midstate derives its two).
struct ellswift_midstate { u32 s[8]; };
S2K_HD void ellswift_tag_midstate(ellswift_midstate& m) {
    const char* tag = "secp256k1_ellswift_encode";
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)tag, 25);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);               // exactly one block -> compressed
    for (int i = 0; i < 8; i++) m.s[i] = g.s[i];
}
// the per-item state: one compression absorbs ser33(P) | 31 zero bytes, put together from words.  P normalised.
S2K_HD void ellswift_key_state(u32 st[8], const ellswift_midstate& mid, const ge& P) {
    u32 xl[8], w[16];
    fe_to_words(xl, P.x);
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = mid.s[j];
    w[0] = ((u32)(2 + fe_is_odd(P.y)) << 24) | (xl[7] >> 8);
#pragma unroll
    for (int j = 1; j < 8; j++) w[j] = (xl[8 - j] << 24) | (xl[7 - j] >> 8);
    w[8] = xl[0] << 24;
#pragma unroll
    for (int j = 9; j < 16; j++) w[j] = 0;
    sha256_compress(st, w);
}
// one draw: the compression of rnd32 | LE32(cnt) | padding behind the item's state; (64 + 64 + 36) bytes were hashed in all
S2K_HD void ellswift_draw(u32 out[8], const u32 st[8], const u32 rnd[8], u32 cnt) {
    u32 w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = rnd[j]; out[j] = st[j]; }
    w[8] = ((cnt & 0xFFu) << 24) | ((cnt & 0xFF00u) << 8) | ((cnt >> 8) & 0xFF00u) | (cnt >> 24);
    w[9] = 0x80000000u;
#pragma unroll
    for (int j = 10; j < 15; j++) w[j] = 0;
    w[15] = 8u * (64u + 64u + 36u);
    sha256_compress(out, w);
}
// The counter schedule of :333-367.  Attempts count from 0.  Counter 65 j refills the pool of 64 branch values that serves attempts
// 64 j .. 64 j + 63, so attempt a draws its u from counter a + a / 64 + 1; branch value k of a pool (k = a mod 64) sits in byte
// (63 - k) >> 1 of the pool hash, shifted by ((63 - k) & 1) << 2, and its top bit is dropped.
S2K_HD u32 ellswift_pool_counter(u32 attempt) { return 65u * (attempt >> 6); }
S2K_HD u32 ellswift_draw_counter(u32 attempt) { return attempt + (attempt >> 6) + 1u; }
S2K_HD void ellswift_branch_index(u32& byte, u32& shift, u32 attempt) {
    const u32 left = 63u - (attempt & 63u);
    byte = left >> 1; shift = (left & 1u) << 2;
}
// pool: the pool hash as 8 big-endian words
S2K_HD int ellswift_branch_value(const u32 pool[8], u32 attempt) {
    u32 byte, shift, word = 0;
    ellswift_branch_index(byte, shift, attempt);
#pragma unroll
    for (u32 j = 0; j < 8; j++) word = ((byte >> 2) == j) ? pool[j] : word;
    return (int)(((word >> (24u - 8u * (byte & 3u))) >> shift) & 7u);
}

// secp256k1_ellswift_encode for one item, one item per lane: the plain form of the loop.  Every lane of a wavefront runs attempt a at
// the same time (the pool refill is uniform); the loop goes on while any lane of the wavefront is unfinished, and a finished lane
// keeps walking with `active` 0, i.e. 1 into the shared inversion.  A lane takes its FIRST success, so the output is the reference's.
// key_format 1: the 64-byte secp256k1_pubkey object (an all-zero x gives 0: the reference's illegal-argument callback); 2: 33 bytes as
// secp256k1_ec_pubkey_parse accepts and refuses them.  Returns 1 and ell64 = u32 | ser32(t) with u32 the raw hash output (not the
// reduced u) and t of the parity of y (:375-382), or 0 and 64 zero bytes: a refused key, or -- *capped = 1 -- an item that found
// nothing in max_attempts (<= ELLSWIFT_MAX_ATTEMPTS) attempts.  Nothing is written when !live.
S2K_HD int ellswift_encode_lane(unsigned char* ell64_out, int* capped, const ellswift_midstate& mid, const unsigned char* key, int key_format,
                                const unsigned char* rnd32, int live, u32 max_attempts) {
    ge P;
    const int ok = live & tweak_key_load(P, key, key_format);
    fe_normalize(P.x); fe_normalize(P.y);
    const int y_odd = fe_is_odd(P.y);                                              // (all that is kept of y across the loop)
    u32 st[8], rnd[8], pool[8];
    ellswift_key_state(st, mid, P);
#pragma unroll
    for (int j = 0; j < 8; j++) { rnd[j] = s2k_load_be32(rnd32 + 4 * j); pool[j] = 0; }
    fe t; fe_set_zero(t);
    int found = 0;
    u32 hit_at = 0;
#pragma unroll 1
    for (u32 a = 0; a < max_attempts && S2K_WAVE_ANY(ok & !found); a++) {
        if ((a & 63u) == 0u) ellswift_draw(pool, st, rnd, ellswift_pool_counter(a));
        const int c = ellswift_branch_value(pool, a);
        u32 h[8], v[8];
        ellswift_draw(h, st, rnd, ellswift_draw_counter(a));
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = h[7 - j];
        fe u, tt; fe_from_words(u, v);                                             // secp256k1_fe_set_b32_mod
        const int active = ok & !found;
        const int hit = ellswift_xswiftec_inv(tt, P.x, u, c, active) & !fe_normalizes_to_zero(u);     // (u = 0: the reference asserts it away; here the attempt fails)
        fe_cmov(t, tt, hit);
        hit_at = hit ? a : hit_at;
        found |= hit;
    }
    *capped = ok & !found;
    fe nt;
    fe_normalize(t);
    fe_neg(nt, t, 1); fe_normalize(nt);
    fe_cmov(t, nt, fe_is_odd(t) != y_odd);
    if (live) {
        if (found) {
            u32 uw[8];
            ellswift_draw(uw, st, rnd, ellswift_draw_counter(hit_at));             // (drawn again: one compression instead of eight registers held across the loop)
#pragma unroll
            for (int j = 0; j < 8; j++) s2k_store_be32(ell64_out + 4 * j, uw[j]);
            fe_get_b32(ell64_out + 32, t);
        } else for (int i = 0; i < 64; i++) ell64_out[i] = 0;
    }
    return found;
}
