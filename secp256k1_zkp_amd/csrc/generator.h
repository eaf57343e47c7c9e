// generator.h -- asset generators and explicit-amount commitments, one item per lane.
//   generate  (secp256k1_generator_generate / _generate_blinded, src/modules/generator/main_impl.h:204-264):
//       gen = [blind*G +] map(SHA256("1st generation: " | key)) + map(SHA256("2nd generation: " | key)),
//       map = shallue_van_de_woestijne (:94-202)
//   parse / serialize (secp256k1_generator_parse :59-77, secp256k1_generator_serialize :79-92)
//   commit    (secp256k1_pedersen_commit :309-335, secp256k1_pedersen_ecmult pedersen_impl.h:42-49):
//       commit = blind*G + value*gen, serialised with prefix 9 ^ is_square(y)
// PUBLIC INPUTS ONLY.  The reference's generate_blinded and pedersen_commit are secret-key paths and constant time; nothing in here
// is: a blind handed to these routines is treated as public data (the explicit-amount case, blind = 0, and re-derivation of public
// generators are what they are for).
// The map is followed as the reference writes it -- constants negc and d, joint denominator j = (8 + t^2)(-3 t^2), candidates in the
// order x1, x2, x3, the root fe_sqrt returns, y negated when t is odd -- with one difference in where the inversions happen: 1/j of
// the two maps of an item is ONE wave-shared inversion of j1*j2 (fe_inv_lanes, waveinv.h), and the to-affine step is a second one.  The
// reference's fe_inv(0) = 0 is part of the map (t = 0 gives (d, f(d))) while fe_inv_lanes(0) poisons the wavefront, so a lane with
// j == 0 hands in 1 and takes 0 as its inverse.  No lane may leave in front of either inversion.
// One fe_sqrt body serves all six roots of an item: the candidates go through a rolled loop and so do the two maps.
#pragma once
#include "tweak.h"        // tweak_gmul_fixed, tweak_affine_lane; ecdsa.h -> ecmult.h, waveinv.h
#include "sha256.h"

// -sqrt(-3) and (sqrt(-3) - 1) / 2  (main_impl.h:131-132)
S2K_HD void gen_fe_negc(fe& r) {
    const u32 w[8] = {0xe32a03ddu, 0x8272d850u, 0x25eb132bu, 0x39e092eau, 0x586869d3u, 0xdcc88f3du, 0xcaf80e20u, 0xf5d2d456u};
    fe_from_words(r, w);
}
S2K_HD void gen_fe_d(fe& r) {
    const u32 w[8] = {0x8e6afa40u, 0x3ec693d6u, 0xed0a766au, 0x630fb68au, 0x53cbcb16u, 0x919bb861u, 0x9a83f8efu, 0x851695d4u};
    fe_from_words(r, w);
}

// t2 = t^2, wd = 8 + t^2 (magnitude 1), x3d = -3 t^2 (magnitude 4)
S2K_HD void gen_map_denoms(fe& t2, fe& wd, fe& x3d, const fe& t) {
    fe_sqr(t2, t);
    x3d = t2; fe_mul_int(x3d, 3); fe_neg(x3d, x3d, 3);
    wd = t2; wd.n[0] += 8u;
}
// j = wd * x3d: zero only for t = 0 (-8 is not a square)
S2K_HD void gen_map_j(fe& j, const fe& t) {
    fe t2, wd, x3d;
    gen_map_denoms(t2, wd, x3d, t);
    fe_mul(j, wd, x3d);
}
// shallue_van_de_woestijne(t) given jinv = 1/j, or 0 where j == 0.  t normalised (its oddness is read).  Which candidate was taken
// comes back in *branch (0, 1, 2 for x1, x2, x3) when asked for.  r: magnitudes (1, 1).
S2K_HD void gen_map_point(ge& r, const fe& t, const fe& jinv, int* branch = nullptr) {
    fe x1, x3;
    {
        fe t2, wd, x3d, negc, d;
        gen_map_denoms(t2, wd, x3d, t);
        gen_fe_negc(negc); gen_fe_d(d);
        fe_mul_sqr(x1, negc, t2, x3, wd);              // -c t^2, wd^2
        fe_mul2(x1, x1, x3d, x3, x3, wd);              // -c t^2 x3d, wd^3
        fe_mul2(x1, x1, jinv, x3, x3, jinv);
        fe_add(x1, d); fe_norm_weak(x1);               // x1 = d - c t^2 x3d / j
        x3.n[0] += 1u; fe_norm_weak(x3);               // x3 = 1 + wd^3 / j
    }
    int aq = 0, bq = 0;
    fe_set_zero(r.x); fe_set_zero(r.y);
#pragma unroll 1
    for (int k = 0; k < 3; k++) {                      // rolled: one fe_sqrt body
        fe x = x1, c, y;
        if (k == 1) { x.n[0] += 1u; fe_neg(x, x, 1); fe_norm_weak(x); }      // x2 = -(x1 + 1)
        fe_cmov(x, x3, k == 2);
        ge_curve_rhs(c, x); fe_norm_weak(c);
        const int q = fe_sqrt(y, c);
        const int take = (k == 0) | ((k == 1) & !aq & q) | ((k == 2) & !aq & !bq);
        fe_cmov(r.x, x, take); fe_cmov(r.y, y, take);
        aq |= (k == 0) & q; bq |= (k == 1) & q;
    }
    if (branch) *branch = aq ? 0 : (bq ? 1 : 2);
    fe ny; fe_neg(ny, r.y, 1);
    fe_cmov(r.y, ny, fe_is_odd(t));
    fe_norm_weak(r.y);
}

// SHA256(prefix16 | key32) as a field element: one block (48 bytes of message, the padding and the length fit behind them).
// which 0: "1st generation: ", 1: "2nd generation: ".  Returns 0 when the hash is >= p (secp256k1_fe_set_b32_limit).
S2K_HD int gen_hash_to_fe(fe& t, int which, const unsigned char* key32) {
    u32 s[8], w[16];
    sha256_init(s);
    w[0] = which ? 0x326e6420u : 0x31737420u; w[1] = 0x67656e65u; w[2] = 0x72617469u; w[3] = 0x6f6e3a20u;
#pragma unroll
    for (int i = 0; i < 8; i++) w[4 + i] = s2k_load_be32(key32 + 4 * i);
    w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = 48u * 8u;
    sha256_compress(s, w);
    u32 v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = s[7 - j];
    fe_from_words(t, v);
    const u32 hi = v[2] & v[3] & v[4] & v[5] & v[6] & v[7];
    const int ge_p = (hi == 0xFFFFFFFFu) && (v[1] == 0xFFFFFFFFu || (v[1] == 0xFFFFFFFEu && v[0] >= 0xFFFFFC2Fu));
    return !ge_p;
}

// Part 1: R = [blind*G +] map(t1) + map(t2), in the reference's order of additions (main_impl.h:216-243).  blind32 NULL: no blind
// (the same for every lane of a launch).  The first inversion of the wavefront is in here.  Equal points double, as the reference's
// complete addition does; opposite points (undefined in the reference) leave R at infinity and the verdict 0.
S2K_HD int generator_sum_lane(gej& R, const fe& t1, const fe& t2, const unsigned char* blind32, int ok, const u32* gtab) {
    gej acc; gej_set_infinity(acc);
    if (blind32) {
        int ov; scalar b;
        sc_set_b32(b, blind32, &ov); ok &= !ov;                   // blind >= n: the reference reduces it and returns 0; here 0 and no generator
        if (!ok) sc_set_zero(b);
        tweak_gmul_fixed(acc, gtab, b.d);
    }
    fe ji1, ji2;
    {
        fe j1, j2, one, J, Ji;
        gen_map_j(j1, t1); gen_map_j(j2, t2);
        const int z1 = fe_normalizes_to_zero(j1), z2 = fe_normalizes_to_zero(j2);
        fe_set_int(one, 1);
        fe_cmov(j1, one, z1); fe_cmov(j2, one, z2);
        fe_mul(J, j1, j2);
        ok &= fe_inv_lanes(Ji, J);
        fe_mul2(ji1, Ji, j2, ji2, Ji, j1);
        fe zero; fe_set_zero(zero);
        fe_cmov(ji1, zero, z1); fe_cmov(ji2, zero, z2);
    }
#pragma unroll 1
    for (int k = 0; k < 2; k++) {                                 // rolled: the map is one routine used twice
        fe t = t1, ji = ji1;
        fe_cmov(t, t2, k); fe_cmov(ji, ji2, k);
        ge p; gen_map_point(p, t, ji);
        gej s; const int f = gej_add_ge(s, acc, p);
        if (S2K_WAVE_ANY(f == GEJ_ADD_NEEDS_DOUBLE)) {
            gej d; gej_double(d, s);
            if (f == GEJ_ADD_NEEDS_DOUBLE) s = d;
        }
        acc = s;
    }
    R = acc;
    ok &= !R.inf;
    return ok;
}
// Returns 1 and the 64-byte secp256k1_generator object (x | y big-endian, secp256k1_generator_save :51-57), or 0 and 64 zero bytes.
// t1, t2 normalised.  Nothing is written when !live.  Both wave-shared inversions are in here: EVERY lane of the wavefront comes through.
S2K_HD int generator_from_t_lane(unsigned char* gen_out64, const fe& t1, const fe& t2, const unsigned char* blind32, int ok, int live, const u32* gtab) {
    gej R; ge a;
    ok &= live;
    ok = generator_sum_lane(R, t1, t2, blind32, ok, gtab);
    ok = tweak_affine_lane(a, R, ok);
    if (live) {
        if (ok) { fe_get_b32(gen_out64, a.x); fe_get_b32(gen_out64 + 32, a.y); }
        else for (int i = 0; i < 64; i++) gen_out64[i] = 0;
    }
    return ok;
}
// secp256k1_generator_generate (blind32 NULL) / secp256k1_generator_generate_blinded
S2K_HD int generator_generate_lane(unsigned char* gen_out64, const unsigned char* key32, const unsigned char* blind32, int live, const u32* gtab) {
    fe t1, t2;
    int ok = gen_hash_to_fe(t1, 0, key32);
    ok &= gen_hash_to_fe(t2, 1, key32);
    return generator_from_t_lane(gen_out64, t1, t2, blind32, ok, live, gtab);
}

// secp256k1_generator_parse: prefix 0x0a / 0x0b, x < p, x on the curve; the y that is a square, negated for 0x0b.
S2K_HD int generator_parse_lane(unsigned char* gen_out64, const unsigned char* in33, int live) {
    fe x; ge g;
    int ok = live & ((in33[0] & 0xFE) == 10);
    ok &= fe_set_b32_limit(x, in33 + 1);
    ok &= ge_set_xquad(g, x);
    fe_normalize(g.y);
    if (in33[0] & 1) { fe_neg(g.y, g.y, 1); fe_normalize(g.y); }
    if (live) {
        if (ok) { fe_get_b32(gen_out64, g.x); fe_get_b32(gen_out64 + 32, g.y); }
        else for (int i = 0; i < 64; i++) gen_out64[i] = 0;
    }
    return ok;
}
// secp256k1_generator_serialize: prefix 11 ^ is_square(y), then x.  The object is read as it is (secp256k1_generator_load :40-49).
S2K_HD void generator_serialize_lane(unsigned char* out33, const unsigned char* gen64, int live) {
    fe x, y, r;
    fe_set_b32_mod(x, gen64); fe_set_b32_mod(y, gen64 + 32);
    fe_normalize(x);
    const int sq = fe_sqrt(r, y);
    if (live) { out33[0] = (unsigned char)(11 ^ sq); fe_get_b32(out33 + 1, x); }
}

// secp256k1_pedersen_commit: blind*G + value*gen through ecmult_lane (na = value, ng = blind), one wave-shared to-affine inversion,
// one root for the prefix.  blind32 NULL: all-zero blinds, no fixed-base part (the same for every lane of a launch).  Returns 1 and
// the 33 bytes 9 ^ is_square(y) | x, or 0 and 33 zero bytes (blind >= n; the point at infinity: blind = 0 with value = 0, or
// blind*G = -value*gen).  The generator object is read as it is: one that is not on the curve is the caller's error, but the error stays
// with that item: an object with y = 0 (the all-zero object included) is refused, whatever value and blind are, and so is an item whose
// sum comes out with Z = 0 -- 0 and 33 zero bytes, the neighbours in the wavefront untouched; other off-curve objects give some 33 bytes.
S2K_HD int pedersen_commit_lane(unsigned char* commit_out33, const unsigned char* blind32, u64 value, const unsigned char* gen64, int live,
                                const u32* gtab, const lane_mem& lm) {
    int ok = live;
    scalar b, v; sc_set_zero(b); sc_set_zero(v);
    if (blind32) { int ov; sc_set_b32(b, blind32, &ov); ok &= !ov; }
    v.d[0] = (u32)value; v.d[1] = (u32)(value >> 32);
    ge G; fe_set_b32_mod(G.x, gen64); fe_set_b32_mod(G.y, gen64 + 32);
    ok &= !fe_normalizes_to_zero(G.y);                            // no point of the curve has y = 0: the all-zero object and its like are refused
    if (!ok) { sc_set_zero(b); sc_set_zero(v); }
    gej A, R; gej_set_ge(A, G);
    ecmult_lane(R, A, v, b, blind32 != nullptr, gtab, lm);
    ok &= !R.inf;
    ok &= !fe_normalizes_to_zero(R.z);                            // another object off the curve can still end at Z = 0 without the flag (a multiple
    ge a;                                                         // with y = 0 doubles to Z3 = Y Z = 0): its own result is 0, and the shared inversion never sees the zero
    ok = tweak_affine_lane(a, R, ok);
    fe r;
    const int sq = fe_sqrt(r, a.y);
    if (live) {
        if (ok) { commit_out33[0] = (unsigned char)(9 ^ sq); fe_get_b32(commit_out33 + 1, a.x); }
        else for (int i = 0; i < 33; i++) commit_out33[i] = 0;
    }
    return ok;
}
