// pubkey.h -- the public-key group of include/secp256k1.h and include/secp256k1_extrakeys.h, one item per lane, public data only:
//   convert   secp256k1_ec_pubkey_parse (src/secp256k1.c:290-306, src/eckey_impl.h:18-36), secp256k1_ec_pubkey_serialize (:308-332),
//             secp256k1_xonly_pubkey_parse / _serialize / _from_pubkey (src/modules/extrakeys/main_impl.h:22-42, :44-59, :85-116) and
//             the bridge to and from the x | y form of the multiplication entry points: load in one format, store in another
//   negate    secp256k1_ec_pubkey_negate (secp256k1.c:723-736): the same with y negated before the store
//   tweak_mul secp256k1_ec_pubkey_tweak_mul (secp256k1.c:810-831, eckey_impl.h:82-92): t * P through ecmult_lane with a zero ng
//   combine   secp256k1_ec_pubkey_combine (secp256k1.c:843-867): the sum of a set of keys.  Its first pass is here (pubkey_fold_lane: one
//             lane loads up to `fanin` consecutive keys of one set from their bytes and folds them with the mixed addition gej_add_ge,
//             8M + 3S a key and no partial written per key); the further passes are musig_agg.h's segmented fold over the same plan
//             (musig_agg_plan_sum), the finish is pubkey_combine_finish_lane.  Formats 0 and 2, a square root per key, go one key per
//             lane to a partial first (pubkey_partial_lane) and through every pass of the fold: F roots in a row in one lane lose to
//             one root in each of F lanes.
// Flag-and-select style as tweak.h: an `ok` flag, the scalar of a dead item zeroed, no lane leaves in front of ecmult_lane or the
// wave-shared inversion (which a lane without a result enters with z = 1).  Where a lane's verdict is 0 its output bytes are all zero.
#pragma once
#include "musig_agg.h"    // tweak.h (tweak_key_load, tweak_affine_lane), ecdsa.h, the segmented sum's range and to-affine step
#include "../../include/secp256k1_zkp_amd.h"      // S2K_PK_*

#define PUBKEY_FOLD_FANIN_DEFAULT 16
#define PUBKEY_FOLD_FANIN_MAX 64

S2K_HD int pubkey_in_format_ok(int f) { return f >= S2K_PK_XONLY && f <= S2K_PK_AFFINE; }
S2K_HD int pubkey_out_format_ok(int f) { return f >= S2K_PK_XONLY && f <= S2K_PK_XONLY_OBJECT; }
S2K_HD size_t pubkey_bytes(int f) { return f == S2K_PK_XONLY ? 32 : f == S2K_PK_COMPRESSED ? 33 : f == S2K_PK_FULL ? 65 : 64; }

// Formats 0, 1, 2 are tweak.h's; 3: 65 bytes, 04 / 06 / 07 with the hybrid parity rule (eckey_impl.h:18-36); 4: x | y big-endian,
// accepted iff x < p, y < p and the point is on the curve (defined here: the reference has no such call).  Formats 0 and 2 cost a
// square root, 3 and 4 an on-curve check, 1 nothing.  P comes back with magnitude-1 coordinates, also when the key is refused.
S2K_HD int pubkey_load(ge& P, const unsigned char* key, int format) {
    if (format <= S2K_PK_COMPRESSED) return tweak_key_load(P, key, format);
    if (format == S2K_PK_FULL) return ecdsa_pubkey_load(P, key, ECDSA_PK_FULL);
    int ok = fe_set_b32_limit(P.x, key);
    ok &= fe_set_b32_limit(P.y, key + 32);
    ok &= ge_is_valid(P);
    return ok;
}

// a: normalised.  Format 5 is the object with y made even (secp256k1_xonly_pubkey_from_pubkey); format 0 drops y altogether.
S2K_HD void pubkey_store(unsigned char* out, int format, const ge& a) {
    if (format == S2K_PK_XONLY) {
        fe_get_b32(out, a.x);
    } else if (format == S2K_PK_OBJECT) {
        ecdsa_fe_get_le32(out, a.x); ecdsa_fe_get_le32(out + 32, a.y);
    } else if (format == S2K_PK_COMPRESSED) {
        out[0] = (unsigned char)(2 + fe_is_odd(a.y));
        fe_get_b32(out + 1, a.x);
    } else if (format == S2K_PK_FULL) {
        out[0] = 4;
        fe_get_b32(out + 1, a.x); fe_get_b32(out + 33, a.y);
    } else if (format == S2K_PK_AFFINE) {
        fe_get_b32(out, a.x); fe_get_b32(out + 32, a.y);
    } else {
        fe y = a.y;
        if (fe_is_odd(y)) { fe_neg(y, y, 1); fe_normalize(y); }
        ecdsa_fe_get_le32(out, a.x); ecdsa_fe_get_le32(out + 32, y);
    }
}
// the common tail: the point, or zero bytes; the parity byte is is_odd(y) of the point handed in (for formats 0 and 5 that is the
// parity the encoding drops: pk_parity of secp256k1_xonly_pubkey_from_pubkey).  Nothing is written when !live.
S2K_HD int pubkey_put(unsigned char* out, int out_format, unsigned char* parity_out, const ge& a, int ok, int live) {
    if (!live) return 0;
    if (ok) pubkey_store(out, out_format, a);
    else { const size_t ob = pubkey_bytes(out_format); for (size_t i = 0; i < ob; i++) out[i] = 0; }
    if (parity_out) *parity_out = ok ? (unsigned char)fe_is_odd(a.y) : (unsigned char)0;
    return ok;
}

// convert / negate
S2K_HD int pubkey_convert_lane(unsigned char* out, int out_format, unsigned char* parity_out, const unsigned char* in, int in_format, int negate, int live) {
    ge P;
    const int ok = live & pubkey_load(P, in, in_format);
    fe_normalize(P.x); fe_normalize(P.y);
    if (negate) { fe_neg(P.y, P.y, 1); fe_normalize(P.y); }
    return pubkey_put(out, out_format, parity_out, P, ok, live);
}

// t * P.  0 for t >= n, t == 0 and a key that does not load; otherwise the product, which is never infinite for a point of the curve
// (an object that is a point off the curve can still end at infinity or at Z = 0 without the flag: 0 as well).  Nothing of the key is
// needed behind the multiplication, so no point is held across it: the load's flag alone.
S2K_HD int pubkey_tweak_mul_lane(unsigned char* out, int out_format, unsigned char* parity_out, const unsigned char* key, int key_format, const unsigned char* tweak32,
                                 int live, const u32* gtab, const lane_mem& lm) {
    int ok = live, ov;
    scalar t, zero; sc_set_zero(zero);
    sc_set_b32(t, tweak32, &ov); ok &= !ov;
    ok &= !sc_is_zero(t);
    gej R;
    {
        ge P;
        ok &= pubkey_load(P, key, key_format);
        if (!ok) sc_set_zero(t);
        gej Pj; gej_set_ge(Pj, P);
        ecmult_lane(R, Pj, t, zero, 0, gtab, lm);
    }
    ok &= !R.inf;
    ok &= !fe_normalizes_to_zero(R.z);
    ge a; ok = tweak_affine_lane(a, R, ok);
    return pubkey_put(out, out_format, parity_out, a, ok, live);
}

// combine, first pass: out = the sum of keys[first .. first + count) as a 28-word partial (count 0: infinity).  An infinite
// accumulator takes the key itself (gej_add_ge does), acc == key is the doubling, acc == -key infinity in mid-chain.  A key that does
// not load is left out of the sum and clears the returned flag.
S2K_HD int pubkey_fold_lane(u32* out28, const unsigned char* keys, int key_format, u64 first, u64 count) {
    const size_t kb = pubkey_bytes(key_format);
    gej acc; gej_set_infinity(acc);
    int ok = 1;
    for (u64 k = 0; k < count; k++) {
        ge P;
        const int good = pubkey_load(P, keys + kb * (size_t)(first + k), key_format);
        ok &= good;
        if (good) {
            gej r;
            const int f = gej_add_ge(r, acc, P);
            if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, r); r = d; }
            acc = r;
        }
    }
    gej_park(out28, 1, acc);
    return ok;
}
// the load-then-fold form of the first pass (formats 0 and 2; every format with -DS2K_PK_FOLD_FUSED=0): one key per lane to a 28-word
// partial (infinity where it does not load) and its flag; musig_agg.h's fold then takes it from pass 0
S2K_HD int pubkey_partial_lane(u32* out28, const unsigned char* key, int key_format) {
    ge P;
    const int ok = pubkey_load(P, key, key_format);
    gej A; gej_set_ge(A, P);
    if (!ok) gej_set_infinity(A);
    gej_park(out28, 1, A);
    return ok;
}
// output j of the first pass under the plan's first two offset arrays: the chunk's keys, through musig_agg_sum_range
S2K_HD int pubkey_fold_item(u32* out, const unsigned char* keys, int key_format, const u64* in_off, const u64* out_off, u64 nseg, u32 fanin, u64 j) {
    u64 first, count;
    musig_agg_sum_range(first, count, in_off, out_off, nseg, fanin, j);
    return pubkey_fold_lane(out + (size_t)MUSIG_AGG_GEJ_WORDS * j, keys, key_format, first, count);
}

// combine, finish: one set per lane.  m: the set's keys; its flags are flag[first .. first + count).  0 for an empty set, a cleared
// flag and a sum at infinity.  EVERY lane of the wavefront comes through here (musig_agg_affine).
S2K_HD int pubkey_combine_finish_lane(unsigned char* out, int out_format, unsigned char* parity_out, const u32* sum28, const int32_t* flag, u64 first, u64 count,
                                      u64 m, int live) {
    int ok = live & (m > 0);
    for (u64 k = 0; k < count; k++) ok &= flag[first + k] != 0;
    ge a; int inf;
    ok = musig_agg_affine(a, &inf, sum28, ok);
    return pubkey_put(out, out_format, parity_out, a, ok, live);
}
