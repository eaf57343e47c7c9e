// tweak.h -- public-key tweak-add and the Taproot commitment check, one item per lane.
//   check (secp256k1_xonly_pubkey_tweak_add_check, src/modules/extrakeys/main_impl.h:135-154):
//       accept  <=>  the key loads, t < n, R = P + t*G is finite, ser32(x(R)) == tweaked32 and is_odd(y(R)) == parity
//   add   (secp256k1_xonly_pubkey_tweak_add, src/modules/extrakeys/main_impl.h:118-133; secp256k1_ec_pubkey_tweak_add,
//          src/secp256k1.c:766-790; both through secp256k1_ec_pubkey_tweak_add_helper / secp256k1_eckey_pubkey_tweak_add,
//          src/eckey_impl.h:62-72):  R = P + t*G as a secp256k1_pubkey object, or 0 and 64 zero bytes
// Nothing variable is multiplied: t*G is one mixed addition per window of the generator table (tweak_gmul_fixed, no doubling), then one
// addition of P and one to-affine step.  Neither ecmult_lane nor its per-lane table or digit stream is used.  Flag-and-select style as
// ecdsa.h: an `ok` flag, the tweak of a dead item zeroed, no lane leaves in front of the wave-shared inversion.
#pragma once
#include "ecdsa.h"        // ecdsa_pubkey_load, ecdsa_fe_get_le32, fe_set_le32 (schnorr.h), fe_inv_lanes (waveinv.h)

#define TWEAK_KEY_XONLY 0
#define TWEAK_KEY_OBJECT 1
#define TWEAK_KEY_COMPRESSED 2

S2K_HD size_t tweak_key_bytes(int key_format) { return key_format == TWEAK_KEY_XONLY ? 32 : key_format == TWEAK_KEY_OBJECT ? 64 : 33; }

// key_format 0: 32 bytes, secp256k1_xonly_pubkey_parse (extrakeys/main_impl.h:22-42: x >= p or x not on the curve fails; the even y);
// 1: the 64-byte object of secp256k1_xonly_pubkey / secp256k1_pubkey as it is -- an odd y stays odd (secp256k1_xonly_pubkey_load is
// secp256k1_pubkey_load); all-zero x, where the reference raises its illegal-argument callback, gives 0; 2: 33 bytes compressed
// (secp256k1_ec_pubkey_parse).  P comes back with magnitude-1 coordinates, also when the key is refused.
S2K_HD int tweak_key_load(ge& P, const unsigned char* key, int key_format) {
    if (key_format == TWEAK_KEY_XONLY) {
        fe x; int ok = fe_set_b32_limit(x, key);
        ok &= ge_set_xo(P, x, 0);
        fe_norm_weak(P.y);
        return ok;
    }
    return ecdsa_pubkey_load(P, key, key_format == TWEAK_KEY_OBJECT ? ECDSA_PK_OBJECT : ECDSA_PK_COMPRESSED);
}

// word i of a recoded scalar, i not known at compile time: selects over constant indices, so that the words stay in registers
S2K_HD u32 tweak_recoded_word(const u32 kr[S2K_GTAB_SWORDS], u32 i) {
    u32 r = 0;
#pragma unroll
    for (u32 j = 0; j < S2K_GTAB_SWORDS; j++) r = (i == j) ? kr[j] : r;
    return r;
}
// window g of the recoded scalar -> the record to add (returns 0: the digit is zero) and whether its y is negated
S2K_HD int tweak_window(const u32*& rec, int& neg, const u32* tab, const gtab_geom& G, const u32 kr[S2K_GTAB_SWORDS], int g) {
    const u32 word = ((u32)g * G.D) >> 5;
    return gtab_locate(rec, neg, tab, G, g, tweak_recoded_word(kr, word), tweak_recoded_word(kr, word + 1u));
}
// out = k * G through the fixed-base table `tab` (k: 8 little-endian words; the table's header gives the geometry, so every width works):
// one gtab_recode, then one gtab_locate and one gej_add_ge per window and no doubling; the record of window w + 1 is requested before the
// addition of window w, so its latency lies under ~11 products.  No addition in here is exceptional: the partial sum S of the windows
// below w has |S| < 2^(D w) / 2, less than the smallest multiple v 2^(D w) window w holds, so S = +-v 2^(D w) is out, and S + v 2^(D w)
// = 0 (mod n) would make the scalar 0, whose digits are all zero.  What is left is S - v B = -n in the top window (B = 2^(D (W-1))):
// it needs S = -(n mod B) with n mod B < B / 2, and bits 129 .. 255 of n are all ones, so n mod B > B / 2 for every width the table
// can have (B >= 2^230).  (The caller's addition of P afterwards can be exceptional.)
S2K_HD void tweak_gmul_fixed(gej& out, const u32* tab, const u32* k8) {
    gej acc; gej_set_infinity(acc);
    const gtab_geom GG = gtab_geometry(tab);
    u32 kr[S2K_GTAB_SWORDS]; gtab_recode(kr, k8, tab);
    u32 raw[16]; int neg = 0;
    const u32* rec = tab;
    int have = tweak_window(rec, neg, tab, GG, kr, 0);
    if (have) {
#pragma unroll
        for (int i = 0; i < 16; i++) raw[i] = rec[i];
    }
#pragma unroll 1
    for (int w = 0; w < (int)GG.W; w++) {
        u32 nraw[16]; int nhave = 0, nneg = 0;
        if (w + 1 < (int)GG.W) {
            const u32* nrec = tab;
            nhave = tweak_window(nrec, nneg, tab, GG, kr, w + 1);
            if (nhave) {
#pragma unroll
                for (int i = 0; i < 16; i++) nraw[i] = nrec[i];
            }
        }
        if (have) {
            ge p; fe_from_words(p.x, raw); fe_from_words(p.y, raw + 8);
            if (neg) { fe_neg(p.y, p.y, 1); fe_norm_weak(p.y); }
            gej t; gej_add_ge(t, acc, p); acc = t;
        }
        have = nhave; neg = nneg;
        if (nhave) {
#pragma unroll
            for (int i = 0; i < 16; i++) raw[i] = nraw[i];
        }
    }
    out = acc;
}

// Part 1: key and tweak in, R = P + t*G out (Jacobian).  Returns 1 iff the key loaded, t < n and R is finite.
S2K_HD int tweak_sum_lane(gej& R, const unsigned char* key, int key_format, const unsigned char* tweak32, int live, const u32* gtab) {
    int ok = live, ov;
    ge P; scalar t;
    sc_set_b32(t, tweak32, &ov); ok &= !ov;                      // t >= n: secp256k1_ec_pubkey_tweak_add_helper fails; t == 0 is legal
    if (!ok) sc_set_zero(t);
    gej T; tweak_gmul_fixed(T, gtab, t.d);
    ok &= tweak_key_load(P, key, key_format);                    // (after the window loop: P's 18 registers are not held across it)
    // T infinite (t == 0): R = P; T == P: the doubling; T == -P: infinity
    const int f = gej_add_ge(R, T, P);
    if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, R); R = d; }
    ok &= !R.inf;
    return ok;
}
// Part 2: to affine, normalised.  fe_inv_lanes is one inversion per wavefront on the device, so EVERY lane of the wavefront must come
// through here; a lane without a finite result hands in z = 1.  A zero return of the inversion clears the lane's verdict.
S2K_HD int tweak_affine_lane(ge& a, const gej& R, int ok) {
    fe z = R.z, one, zi;
    fe_set_int(one, 1);
    fe_cmov(z, one, !ok);
    ok &= fe_inv_lanes(zi, z);
    ge_set_gej_zinv(a, R, zi);
    return ok;
}

// Returns 1 iff secp256k1_xonly_pubkey_tweak_add_check would.  parity other than 0 or 1 gives 0 (the reference compares an int).
// key_format 0 or 1.
S2K_HD int tweak_check_lane(const unsigned char* tweaked32, unsigned parity, const unsigned char* key, int key_format, const unsigned char* tweak32,
                            int live, const u32* gtab) {
    gej R; ge a;
    int ok = tweak_sum_lane(R, key, key_format, tweak32, live, gtab);
    ok = tweak_affine_lane(a, R, ok);
    u32 w[8]; fe_to_words(w, a.x);
    u32 diff = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) diff |= w[7 - j] ^ (((u32)tweaked32[4 * j] << 24) | ((u32)tweaked32[4 * j + 1] << 16) | ((u32)tweaked32[4 * j + 2] << 8) | (u32)tweaked32[4 * j + 3]);
    ok &= diff == 0u;
    ok &= (unsigned)fe_is_odd(a.y) == parity;
    return ok;
}
// Returns 1 and R as a 64-byte secp256k1_pubkey object (the layout ecdsa_recover_lane writes, what key_format 1 reads), or 0 and 64
// zero bytes.  Nothing is written when !live.  key_format 0, 1 or 2.
S2K_HD int tweak_add_lane(unsigned char* pubkey_out64, const unsigned char* key, int key_format, const unsigned char* tweak32, int live, const u32* gtab) {
    gej R; ge a;
    int ok = tweak_sum_lane(R, key, key_format, tweak32, live, gtab);
    ok = tweak_affine_lane(a, R, ok);
    if (live) {
        if (ok) { ecdsa_fe_get_le32(pubkey_out64, a.x); ecdsa_fe_get_le32(pubkey_out64 + 32, a.y); }
        else for (int i = 0; i < 64; i++) pubkey_out64[i] = 0;
    }
    return ok;
}
