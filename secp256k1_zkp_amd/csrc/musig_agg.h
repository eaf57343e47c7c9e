// musig_agg.h -- the rest of the MuSig2 coordinator's flow, all of it public data:
//   key aggregation   (secp256k1_musig_pubkey_agg, src/modules/musig/keyagg_impl.h:156-215): the 197-byte cache and the x-only key of a key set
//   the cache tweaks  (secp256k1_musig_pubkey_ec_tweak_add / _xonly_tweak_add, keyagg_impl.h:231-273)
//   nonce aggregation (secp256k1_musig_nonce_agg, session_impl.h:493-531): the two column sums of a session's pubnonces
//   signature aggregation (secp256k1_musig_partial_sig_agg, session_impl.h:779-805): fin_nonce | s_part + sum of s_i
// Key aggregation is four stages, each a lane function here and a kernel in engine_musig_agg.hip:
//   (a) musig_agg_list_lane    one SET per lane: the "KeyAgg list" hash over the compressed encodings and the index of the second key (the
//                              first key whose bytes differ from key 0's).  Encodings and comparisons come from the key bytes alone: no
//                              square root here.  A key that will not parse is hashed as it stands; stage (d) refuses its set.
//   (b) musig_agg_term_lane    one KEY per lane, flat over all sets: load the key, its coefficient hash, a_i * P_i through ecmult_lane
//                              (coefficient 1 -- a key equal to the second key -- is a select afterwards, and a zeroed scalar where
//                              the whole wavefront has nothing to multiply), a 28-word Jacobian partial and an ok flag
//   (c) musig_agg_fold_lane    one OUTPUT per lane: up to `fanin` consecutive partials of one segment folded with gej_add_var (equal keys
//                              are doublings there); the host repeats the pass until every segment is one partial
//   (d) musig_agg_finish_lane  one SET per lane: AND of the key flags, to affine through the wave-shared inversion, the cache and the key
// Nonce aggregation uses (c) over its two columns between a load stage (one pubnonce per lane) and a finish stage (one session per lane).
// Flag-and-select style as musig.h: an `ok` flag, the scalar of a dead item zeroed, no lane leaves in front of fe_inv_lanes (which a
// dead lane enters with z = 1), and no point is held across the multiplication: stage (b) reads the key again after it.
// Partials are 28 words, contiguous: x | y | z (9 limbs each, magnitude 1) | infinity flag -- gej_park with stride 1.
#pragma once
#include "musig.h"

#define MUSIG_AGG_FANIN_DEFAULT 64
#define MUSIG_AGG_FANIN_MAX 64
#define MUSIG_AGG_NO_SECOND 0xFFFFFFFFu
#define MUSIG_AGG_GEJ_WORDS S2K_PARK_GEJ_WORDS

// segment of item i under the offsets off[0 .. nseg]: the k with off[k] <= i < off[k+1] (empty segments are stepped over).
// Requires off[0] <= i < off[nseg].
S2K_HD u64 musig_agg_segment(const u64* off, u64 nseg, u64 i) {
    u64 lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// what the second-key search compares (the reference: memcmp of the 64-byte objects): format 0 the 33 bytes, format 1 the 64 bytes,
// format 2 bytes 1..64, so that a hybrid encoding of the same point is the same key
S2K_HD int musig_agg_key_same(const unsigned char* a, const unsigned char* b, int pk_format) {
    const int at = pk_format == ECDSA_PK_COMPRESSED ? 0 : pk_format == ECDSA_PK_OBJECT ? 0 : 1;
    const int len = pk_format == ECDSA_PK_COMPRESSED ? 33 : 64;
    unsigned diff = 0;
    for (int i = 0; i < len; i++) diff |= (unsigned)(a[at + i] ^ b[at + i]);
    return diff == 0;
}
// the compressed encoding of a key from its bytes alone
S2K_HD void musig_agg_put33(sha256_stream& h, const unsigned char* k, int pk_format) {
    if (pk_format == ECDSA_PK_COMPRESSED) {
        for (int i = 0; i < 33; i++) sha256_stream_put(h, k[i]);
    } else if (pk_format == ECDSA_PK_OBJECT) {               // x, y as 32 little-endian bytes each
        sha256_stream_put(h, (unsigned char)(2 + (k[32] & 1)));
        for (int i = 0; i < 32; i++) sha256_stream_put(h, k[31 - i]);
    } else {                                                 // 04 / 06 / 07 | x | y, big-endian
        sha256_stream_put(h, (unsigned char)(2 + (k[64] & 1)));
        for (int i = 0; i < 32; i++) sha256_stream_put(h, k[1 + i]);
    }
}

// SHA256 states after the 64-byte tag prefixes "KeyAgg list" and "KeyAgg coefficient" (the reference has both as constants,
// keyagg_impl.h:64-70 and :93-99)
struct musig_agg_mids { u32 list[8], coef[8]; };
S2K_HD void musig_agg_midstates(musig_agg_mids& m) {
    musig_tag_midstate(m.list, "KeyAgg list", 11);
    musig_tag_midstate(m.coef, "KeyAgg coefficient", 18);
}

// (a) the set's keys are pubkeys[first .. first + m).  Writes pks_hash (32 bytes) and the second key's index within the set, or
// MUSIG_AGG_NO_SECOND.  An empty set gets the hash of nothing; stage (d) refuses it.
S2K_HD void musig_agg_list_lane(unsigned char* pks_hash32, u32* second, const u32 mid_list[8], const unsigned char* pubkeys, int pk_format, u64 first, u64 m) {
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    sha256_stream h; musig_hash_start(h, mid_list);
    u32 sec = MUSIG_AGG_NO_SECOND;
    const unsigned char* const k0 = pubkeys + pkb * first;
    for (u64 k = 0; k < m; k++) {
        const unsigned char* const kk = pubkeys + pkb * (first + k);
        musig_agg_put33(h, kk, pk_format);
        if ((sec == MUSIG_AGG_NO_SECOND) & (k > 0)) { if (!musig_agg_key_same(k0, kk, pk_format)) sec = (u32)k; }
    }
    sha256_stream_finalize(h, pks_hash32);
    *second = sec;
}

// (b) key `key` of the flat key array, in the set whose first key is `set_first`, whose second key has index `second` in the set and
// whose list hash is pks_hash32.  Writes the partial a * P (infinity for a key that does not load) where `live`; returns the key's flag.
S2K_HD int musig_agg_term_lane(u32* out28, const u32 mid_coef[8], const unsigned char* pubkeys, int pk_format, u64 key, u64 set_first, u32 second,
                               const unsigned char* pks_hash32, int live, const u32* gtab, const lane_mem& lm) {
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    int ok = live, unit = 0;
    gej T;
    {
        const unsigned char* const pk = pubkeys + pkb * (key + s2k_opaque_zero());
        ge P;
        ok &= ecdsa_pubkey_load(P, pk, pk_format);
        fe_normalize(P.x); fe_normalize(P.y);
        if (second != MUSIG_AGG_NO_SECOND) unit = musig_agg_key_same(pk, pubkeys + pkb * (set_first + second), pk_format);
        scalar mu, zero; sc_set_zero(zero);
        sha256_stream h; musig_hash_start(h, mid_coef);
        sha256_stream_write(h, pks_hash32, 32);
        musig_write_ext33(h, P, 0);
        musig_hash_scalar(mu, h);
        // A key whose coefficient is 1 multiplies along with its wavefront and the product is dropped below: ecmult_lane keeps a
        // wavefront on its lock-step path only while every lane multiplies.  Where no lane of the wavefront has anything to multiply
        // (the second keys of 2-key sets, which the kernel's lane order brings together) every scalar is zero and the call does nothing.
        if (S2K_WAVE_ALL(unit | !ok) | !ok) sc_set_zero(mu);
        gej Pj; gej_set_ge(Pj, P);
        ecmult_lane(T, Pj, mu, zero, 0, gtab, lm);
    }
    if (unit) {                                              // coefficient 1: the key itself, read again
        const unsigned char* const pk = pubkeys + pkb * (key + s2k_opaque_zero());
        ge P; (void)ecdsa_pubkey_load(P, pk, pk_format);
        fe_normalize(P.x); fe_normalize(P.y);
        gej_set_ge(T, P);
    }
    if (!ok) gej_set_infinity(T);
    if (live) gej_park(out28, 1, T);
    return ok;
}

// (c) out = sum of the `count` partials in28[first ..]; count 0 gives infinity
S2K_HD void musig_agg_fold_lane(u32* out28, const u32* in28, u64 first, u64 count) {
    gej acc; gej_set_infinity(acc);
    for (u64 k = 0; k < count; k++) {
        gej t, r;
        gej_unpark(t, in28 + (size_t)MUSIG_AGG_GEJ_WORDS * (first + k), 1);
        gej_add_var(r, acc, t);
        acc = r;
    }
    gej_park(out28, 1, acc);
}

// output j of a pass: segment k of the pass's output offsets, folding inputs in_off[k] + fanin * (j - out_off[k]) ... of that segment
// (the range alone, for a pass that reads something other than partials: pubkey.h's first pass over key bytes)
S2K_HD void musig_agg_sum_range(u64& first, u64& count, const u64* in_off, const u64* out_off, u64 nseg, u32 fanin, u64 j) {
    const u64 k = musig_agg_segment(out_off, nseg, j);
    first = in_off[k] + (u64)fanin * (j - out_off[k]);
    const u64 left = in_off[k + 1] > first ? in_off[k + 1] - first : 0;
    count = left < fanin ? left : fanin;
}
S2K_HD void musig_agg_sum_item(u32* out, const u32* in, const u64* in_off, const u64* out_off, u64 nseg, u32 fanin, u64 j) {
    u64 first, count;
    musig_agg_sum_range(first, count, in_off, out_off, nseg, fanin, j);
    musig_agg_fold_lane(out + (size_t)MUSIG_AGG_GEJ_WORDS * j, in, first, count);
}

// a Jacobian sum to affine through the wave-shared inversion: EVERY lane of the wavefront comes through here.  `want`: the lane has a
// point to convert; a lane without one, an infinite sum and a Z that is 0 without the flag (points off the curve can end there) hand
// in z = 1.  Returns want & finite & the inversion's verdict; *inf is the sum's flag.
S2K_HD int musig_agg_affine(ge& a, int* inf, const u32* sum28, int want) {
    gej S; gej_unpark(S, sum28, 1);
    const int zero_z = fe_normalizes_to_zero(S.z);
    int fin = want & !S.inf & !zero_z;
    fe z = S.z, one, zi; fe_set_int(one, 1);
    fe_cmov(z, one, !fin);
    fin &= fe_inv_lanes(zi, z);
    ge_set_gej_zinv(a, S, zi);
    *inf = S.inf;
    return fin;
}

// (d) the set's sum -> the cache and the x-only key (NULL: not wanted).  Returns 1 iff the set is served; writes 197 (and 64) zero
// bytes where it is not.  Nothing is written when !live.
S2K_HD int musig_agg_finish_lane(unsigned char* cache_out197, unsigned char* agg_pk_out64, const u32* sum28, const int32_t* key_ok, u64 first, u64 m,
                                 const unsigned char* pks_hash32, u32 second, const unsigned char* pubkeys, int pk_format, int live) {
    int ok = live & (m > 0);
    for (u64 k = 0; k < m; k++) ok &= key_ok[first + k] != 0;
    ge a; int inf;
    ok = musig_agg_affine(a, &inf, sum28, ok);
    if (!live) return 0;
    if (!ok) {
        for (int i = 0; i < MUSIG_CACHE_BYTES; i++) cache_out197[i] = 0;
        if (agg_pk_out64) for (int i = 0; i < 64; i++) agg_pk_out64[i] = 0;
        return 0;
    }
    cache_out197[0] = 0xf4; cache_out197[1] = 0xad; cache_out197[2] = 0xbb; cache_out197[3] = 0xdf;
    ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_PK, a.x); ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_PK + 32, a.y);
    if (second != MUSIG_AGG_NO_SECOND) {
        ge S; (void)ecdsa_pubkey_load(S, pubkeys + ecdsa_pk_bytes(pk_format) * (first + second), pk_format);
        fe_normalize(S.x); fe_normalize(S.y);
        ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_SECOND, S.x); ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_SECOND + 32, S.y);
    } else {
        for (int i = 0; i < 64; i++) cache_out197[MUSIG_CACHE_SECOND + i] = 0;
    }
    for (int i = 0; i < 32; i++) cache_out197[MUSIG_CACHE_PKS_HASH + i] = pks_hash32[i];
    for (int i = MUSIG_CACHE_PARITY; i < MUSIG_CACHE_BYTES; i++) cache_out197[i] = 0;
    if (agg_pk_out64) {
        if (fe_is_odd(a.y)) { fe_neg(a.y, a.y, 1); fe_normalize(a.y); }
        ecdsa_fe_get_le32(agg_pk_out64, a.x); ecdsa_fe_get_le32(agg_pk_out64 + 32, a.y);
    }
    return 1;
}

// ---- the cache tweaks: one cache per lane.  xonly_byte: 1 x-only, 0 plain, anything else refuses.  cache_out197 may be cache_in197.
// Returns 1 iff the reference's call would; the output cache (and key) is zero bytes where it does not.  Nothing is written when !live.
S2K_HD int musig_agg_tweak_lane(unsigned char* cache_out197, unsigned char* pubkey_out64, const unsigned char* cache_in197, const unsigned char* tweak32,
                                unsigned xonly_byte, int live, const u32* gtab) {
    int ok = live & MUSIG_MAGIC_CACHE(cache_in197) & (xonly_byte <= 1u), ov;
    scalar t, acc;
    sc_set_b32(t, tweak32, &ov); ok &= !ov;                  // t >= n fails; t == 0 is legal
    if (!ok) sc_set_zero(t);
    gej T; tweak_gmul_fixed(T, gtab, t.d);
    ge P; musig_point_object(P, cache_in197 + MUSIG_CACHE_PK);  // (after the window loop, as tweak_sum_lane)
    unsigned parity = cache_in197[MUSIG_CACHE_PARITY] & 1u;
    sc_set_b32(acc, cache_in197 + MUSIG_CACHE_TWEAK, nullptr);
    if ((xonly_byte == 1u) & fe_is_odd(P.y)) {               // keyagg_impl.h:250-253
        ge n; ge_neg(n, P); P = n;
        parity ^= 1u;
        sc_negate(acc, acc);
    }
    scalar sum; sc_add(sum, acc, t);
    gej R;
    const int f = gej_add_ge(R, T, P);
    if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, R); R = d; }
    ok &= !R.inf;
    ge a; ok = tweak_affine_lane(a, R, ok);
    if (!live) return 0;
    unsigned char keep[96];                                  // second_pk | pks_hash travel as they are (in place: read before the writes)
    for (int i = 0; i < 96; i++) keep[i] = cache_in197[MUSIG_CACHE_SECOND + i];
    if (!ok) {
        for (int i = 0; i < MUSIG_CACHE_BYTES; i++) cache_out197[i] = 0;
        if (pubkey_out64) for (int i = 0; i < 64; i++) pubkey_out64[i] = 0;
        return 0;
    }
    cache_out197[0] = 0xf4; cache_out197[1] = 0xad; cache_out197[2] = 0xbb; cache_out197[3] = 0xdf;
    ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_PK, a.x); ecdsa_fe_get_le32(cache_out197 + MUSIG_CACHE_PK + 32, a.y);
    for (int i = 0; i < 96; i++) cache_out197[MUSIG_CACHE_SECOND + i] = keep[i];
    cache_out197[MUSIG_CACHE_PARITY] = (unsigned char)parity;
    sc_get_b32(cache_out197 + MUSIG_CACHE_TWEAK, sum);
    if (pubkey_out64) { ecdsa_fe_get_le32(pubkey_out64, a.x); ecdsa_fe_get_le32(pubkey_out64 + 32, a.y); }
    return 1;
}

// ---- nonce aggregation
// load: one pubnonce per lane -> its two points as partials (infinity where it is refused) and its flag
S2K_HD int musig_agg_nonce_load_lane(u32* out28_r1, u32* out28_r2, const unsigned char* nonce, int nonce_format, int live) {
    int ok = live & musig_pubnonce_ok(nonce, nonce_format);
    ge R1, R2;
    ok &= musig_pubnonce_point(R1, nonce, nonce_format, 0);
    ok &= musig_pubnonce_point(R2, nonce, nonce_format, 1);
    gej A, B; gej_set_ge(A, R1); gej_set_ge(B, R2);
    if (!ok) { gej_set_infinity(A); gej_set_infinity(B); }
    if (live) { gej_park(out28_r1, 1, A); gej_park(out28_r2, 1, B); }
    return ok;
}
S2K_HD void musig_agg_put_point(unsigned char* out, int object, const ge& a, int inf) {
    if (object) {
        if (inf) { for (int i = 0; i < 64; i++) out[i] = 0; }
        else { ecdsa_fe_get_le32(out, a.x); ecdsa_fe_get_le32(out + 32, a.y); }
    } else {
        unsigned char b[32]; fe_get_b32(b, a.x);
        out[0] = inf ? 0 : (unsigned char)(2 + fe_is_odd(a.y));
        for (int i = 0; i < 32; i++) out[1 + i] = inf ? 0 : b[i];
    }
}
// finish: one session per lane, whose pubnonces are items [first, first + m).  An infinite sum is a valid result.
S2K_HD int musig_agg_nonce_finish_lane(unsigned char* aggnonce_out, int out_format, const u32* sum28_r1, const u32* sum28_r2, const int32_t* nonce_ok,
                                       u64 first, u64 m, int live) {
    int ok = live & (m > 0);
    for (u64 k = 0; k < m; k++) ok &= nonce_ok[first + k] != 0;
    ge a1, a2; int inf1, inf2;
    const int f1 = musig_agg_affine(a1, &inf1, sum28_r1, ok);
    const int f2 = musig_agg_affine(a2, &inf2, sum28_r2, ok);
    ok &= (f1 | inf1) & (f2 | inf2);
    if (!live) return 0;
    const size_t nb = musig_nonce_bytes(out_format);
    if (!ok) { for (size_t i = 0; i < nb; i++) aggnonce_out[i] = 0; return 0; }
    if (out_format == MUSIG_NONCE_OBJECT) {
        aggnonce_out[0] = 0xa8; aggnonce_out[1] = 0xb7; aggnonce_out[2] = 0xe4; aggnonce_out[3] = 0x67;
        musig_agg_put_point(aggnonce_out + 4, 1, a1, inf1); musig_agg_put_point(aggnonce_out + 68, 1, a2, inf2);
    } else {
        musig_agg_put_point(aggnonce_out, 0, a1, inf1); musig_agg_put_point(aggnonce_out + 33, 0, a2, inf2);
    }
    return 1;
}

// ---- signature aggregation: one session per lane over its shares [first, first + m); scalar arithmetic only
S2K_HD int musig_agg_sig_lane(unsigned char* sig64_out, const unsigned char* session133, const unsigned char* partial_sigs, int sig_format, u64 first, u64 m, int live) {
    int ok = live & (m > 0) & MUSIG_MAGIC_SESSION(session133);
    const size_t sgb = musig_sig_bytes(sig_format);
    scalar s; sc_set_b32(s, session133 + MUSIG_SESSION_S_PART, nullptr);
    for (u64 k = 0; k < m; k++) {
        const unsigned char* const sig = partial_sigs + sgb * (first + k);
        scalar t, r;
        if (sig_format == MUSIG_SIG_OBJECT) { ok &= MUSIG_MAGIC_SIG(sig); sc_set_b32(t, sig + 4, nullptr); }
        else { int ov; sc_set_b32(t, sig, &ov); ok &= !ov; }
        sc_add(r, s, t); s = r;
    }
    if (!live) return 0;
    if (!ok) { for (int i = 0; i < 64; i++) sig64_out[i] = 0; return 0; }
    for (int i = 0; i < 32; i++) sig64_out[i] = session133[MUSIG_SESSION_FIN_NONCE + i];
    sc_get_b32(sig64_out + 32, s);
    return 1;
}

// ---- the host's plan of the segmented sum (engine_musig_agg.hip; the host emulation drives its stages from the same plan) ----------------
#include <vector>
#include <algorithm>
// offs holds passes + 1 offset arrays of nseg + 1 entries each.  Array 0 is the input's; a pass turns a segment of length l into one of
// max(1, ceil(l / fanin)) (an empty segment becomes one infinite partial), and after the last pass every segment is one partial:
// result k at index k.  At least one pass runs.  cap: the most partials any array of the chain holds.
struct musig_agg_sum_plan { std::vector<uint64_t> offs; size_t nseg, passes, cap; };
static inline musig_agg_sum_plan musig_agg_plan_sum(const uint64_t* off, size_t nseg, size_t fanin) {
    musig_agg_sum_plan p; p.nseg = nseg; p.passes = 0;
    p.offs.assign(off, off + nseg + 1);
    p.cap = (size_t)off[nseg];
    for (;;) {
        const size_t at = p.passes * (nseg + 1);
        p.offs.resize(p.offs.size() + nseg + 1);
        const uint64_t* in = p.offs.data() + at; uint64_t* out = p.offs.data() + at + nseg + 1;
        uint64_t longest = 0; out[0] = 0;
        for (size_t k = 0; k < nseg; k++) {
            const uint64_t l = in[k + 1] - in[k], o = l == 0 ? 1 : (l + fanin - 1) / fanin;
            out[k + 1] = out[k] + o; longest = std::max(longest, o);
        }
        p.passes++;
        p.cap = std::max(p.cap, (size_t)out[nseg]);
        if (longest <= 1) break;
    }
    return p;
}
// nonce aggregation: the two columns as 2 * n_sessions segments over 2 * n_nonces partials (column 2 of pubnonce i at partial n + i)
static inline musig_agg_sum_plan musig_agg_plan_nonces(const uint64_t* nonce_off, size_t n_sessions, size_t fanin) {
    const uint64_t n = nonce_off[n_sessions];
    std::vector<uint64_t> off(2 * n_sessions + 1);
    for (size_t k = 0; k <= n_sessions; k++) { off[k] = nonce_off[k]; off[n_sessions + k] = n + nonce_off[k]; }
    return musig_agg_plan_sum(off.data(), 2 * n_sessions, fanin);
}
