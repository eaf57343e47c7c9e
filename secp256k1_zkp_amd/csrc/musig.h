// musig.h -- the public-data half of the MuSig2 module, one item per lane.
//   verify  (secp256k1_musig_partial_sig_verify, src/modules/musig/session_impl.h:716-777; the loads :84-186 and keyagg_impl.h:19-60;
//            the key coefficient keyagg_impl.h:93-124):
//       accept  <=>  the four objects carry their magic, the key loads, and  e'*P - s*G + sigma*(R1 + b*R2)  is infinity, where
//                    b, e and the nonce parity come from the session, e' = e*mu negated iff is_odd(y(cache.pk)) != parity_acc,
//                    mu = 1 for the cache's second key and the "KeyAgg coefficient" hash of pks_hash | ser33(P) otherwise,
//                    sigma = -1 iff the session's parity byte is non-zero
//   process (secp256k1_musig_nonce_process, session_impl.h:544-638): aggregate nonce, message and cache in, the 133-byte session out
// Nothing here touches a secret: nonce generation, signing, adapt and extract stay with the reference.  Key aggregation, the cache
// tweaks, nonce aggregation and signature aggregation are musig_agg.h.
// The verifier takes the multi-exponentiation the reference's TODO (:741) asks for: T = (-s)*G + sigma*R1 through the fixed-base table
// (tweak_gmul_fixed, no doubling), J = e'*P + (sigma*b)*R2 through the joint form ecmult_lane2 (128 doublings), or two ecmult_lane calls
// for a wavefront it declines, and the verdict J == -T from one gej_add_var: no inversion.  Flag-and-select style as adaptor.h: an `ok`
// flag, the scalars of dead items zeroed, no early return.  No point is held across a multiplication: T waits in `park`, and every stage
// reads and parses its inputs again from global memory.
#pragma once
#include "tweak.h"        // tweak_gmul_fixed; ecdsa.h: ecdsa_pubkey_load, ecdsa_fe_get_le32; fe_inv_lanes (waveinv.h)
#include "schnorr.h"      // schnorr_midstate: the BIP-340 challenge
#include "gtable.h"       // ge_set_generator
#include "sha256.h"

// 1: J through ecmult_lane2; 0: always the two-call form (the A/B switch of tools/musig_bare.py)
#ifndef S2K_MUSIG_JOINT
#define S2K_MUSIG_JOINT 1
#endif

#define MUSIG_SIG_SERIALIZED 0      /* 32 bytes, as secp256k1_musig_partial_sig_parse: s >= n is refused */
#define MUSIG_SIG_OBJECT 1          /* the 36-byte secp256k1_musig_partial_sig: magic | s, s reduced */
#define MUSIG_NONCE_SERIALIZED 0    /* 66 bytes: two compressed points (pubnonce), or either of them 33 zero bytes (aggnonce only) */
#define MUSIG_NONCE_OBJECT 1        /* the 132-byte object: magic | two 64-byte points */
#define MUSIG_CACHE_BYTES 197
#define MUSIG_SESSION_BYTES 133
// offsets inside the objects (keyagg_impl.h:21-44, session_impl.h:130-152)
#define MUSIG_CACHE_PK 4
#define MUSIG_CACHE_SECOND 68
#define MUSIG_CACHE_PKS_HASH 132
#define MUSIG_CACHE_PARITY 164
#define MUSIG_CACHE_TWEAK 165
#define MUSIG_SESSION_PARITY 4
#define MUSIG_SESSION_FIN_NONCE 5
#define MUSIG_SESSION_B 37
#define MUSIG_SESSION_E 69
#define MUSIG_SESSION_S_PART 101

S2K_HD size_t musig_sig_bytes(int sig_format) { return sig_format == MUSIG_SIG_OBJECT ? 36 : 32; }
S2K_HD size_t musig_nonce_bytes(int nonce_format) { return nonce_format == MUSIG_NONCE_OBJECT ? 132 : 66; }

// per-lane parking area, in words `stride` apart.  verify: T | the fallback's first product.  process: R1 affine (x, y, infinity flag)
#define S2K_MUSIG_PARK_T 0
#define S2K_MUSIG_PARK_FB S2K_PARK_GEJ_WORDS
#define S2K_MUSIG_PARK_WORDS (2 * S2K_PARK_GEJ_WORDS)
#define S2K_MUSIG_PARK_R1_WORDS 19

// SHA256 states after the 64-byte tag prefixes (the reference has the first two as constants, keyagg_impl.h:93-99 and session_impl.h:535-541)
struct musig_midstates { u32 coef[8], noncecoef[8], challenge[8]; };
S2K_HD void musig_tag_midstate(u32 out[8], const char* tag, size_t len) {
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)tag, len);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);     // exactly one block -> compressed
    for (int i = 0; i < 8; i++) out[i] = g.s[i];
}
S2K_HD void musig_tag_midstates(musig_midstates& m) {
    musig_tag_midstate(m.coef, "KeyAgg coefficient", 18);
    musig_tag_midstate(m.noncecoef, "MuSig/noncecoef", 15);
    schnorr_midstate c; schnorr_tag_midstate(c);
    for (int i = 0; i < 8; i++) m.challenge[i] = c.s[i];
}
S2K_HD void musig_hash_start(sha256_stream& h, const u32 mid[8]) {
    for (int i = 0; i < 8; i++) h.s[i] = mid[i];
    for (int i = 0; i < 16; i++) h.buf[i] = 0;
    h.bytes = 64;
}
// the digest as a scalar: mod n, overflow ignored
S2K_HD void musig_hash_scalar(scalar& r, sha256_stream& h) {
    unsigned char d[32];
    sha256_stream_finalize(h, d);
    sc_set_b32(r, d, nullptr);
}
// secp256k1_musig_ge_serialize_ext of a normalised affine point
S2K_HD void musig_write_ext33(sha256_stream& h, const ge& a, int inf) {
    unsigned char b[32]; fe_get_b32(b, a.x);
    sha256_stream_put(h, inf ? 0 : (unsigned char)(2 + fe_is_odd(a.y)));
    for (int i = 0; i < 32; i++) sha256_stream_put(h, inf ? 0 : b[i]);
}
S2K_HD int musig_magic(const unsigned char* p, unsigned m0, unsigned m1, unsigned m2, unsigned m3) {
    return (p[0] == m0) & (p[1] == m1) & (p[2] == m2) & (p[3] == m3);
}
#define MUSIG_MAGIC_PUBNONCE(p) musig_magic(p, 0xf5, 0x7a, 0x3d, 0xa0)
#define MUSIG_MAGIC_AGGNONCE(p) musig_magic(p, 0xa8, 0xb7, 0xe4, 0x67)
#define MUSIG_MAGIC_SESSION(p) musig_magic(p, 0x9d, 0xed, 0xe9, 0x17)
#define MUSIG_MAGIC_SIG(p) musig_magic(p, 0xeb, 0xfb, 0x1a, 0x32)
#define MUSIG_MAGIC_CACHE(p) musig_magic(p, 0xf4, 0xad, 0xbb, 0xdf)
S2K_HD int musig_all_zero(const unsigned char* p, int n) {
    unsigned acc = 0;
    for (int i = 0; i < n; i++) acc |= p[i];
    return acc == 0;
}
// a point inside an object, read as it is (secp256k1_ge_from_bytes): normalised coordinates, nothing refused
S2K_HD void musig_point_object(ge& P, const unsigned char* p64) { (void)ecdsa_pubkey_load(P, p64, ECDSA_PK_OBJECT); }
// point k (0, 1) of a pubnonce; returns 0 where secp256k1_musig_pubnonce_parse would (objects: the magic is the caller's check)
S2K_HD int musig_pubnonce_point(ge& P, const unsigned char* nonce, int nonce_format, int k) {
    if (nonce_format == MUSIG_NONCE_OBJECT) { musig_point_object(P, nonce + 4 + 64 * k); return 1; }
    const int ok = ecdsa_pubkey_load(P, nonce + 33 * k, ECDSA_PK_COMPRESSED);
    fe_normalize(P.y);
    return ok;
}
// what does not depend on a point: the magic of an object (a serialised point gives its verdict in the stage that lifts it)
S2K_HD int musig_pubnonce_ok(const unsigned char* nonce, int nonce_format) { return nonce_format == MUSIG_NONCE_OBJECT ? MUSIG_MAGIC_PUBNONCE(nonce) : 1; }

// mu of signer P (normalised) under the cache: 1 for the second key, the coefficient hash otherwise (secp256k1_musig_keyaggcoef_internal)
S2K_HD void musig_keyagg_coef(scalar& mu, const musig_midstates& mid, const unsigned char* cache, const ge& P) {
    ge S; musig_point_object(S, cache + MUSIG_CACHE_SECOND);
    const int second = (!musig_all_zero(cache + MUSIG_CACHE_SECOND, 64)) & fe_equal(P.x, S.x) & fe_equal(P.y, S.y);
    sha256_stream h; musig_hash_start(h, mid.coef);
    sha256_stream_write(h, cache + MUSIG_CACHE_PKS_HASH, 32);
    musig_write_ext33(h, P, 0);
    musig_hash_scalar(mu, h);
    if (second) sc_set_int(mu, 1);
}

// Term k of J = e'*P + (sigma*b)*R2 for item `it`, read from global memory: k = 0 is (P, e'), k = 1 is (R2, sigma*b).  Returns what the
// loads say about the item (magics, key and nonce parsing, the session index); the scalar is NOT zeroed here.
S2K_HD int musig_verify_term(int k, gej& Pj, scalar& n, const musig_midstates& mid, const unsigned char* nonce, int nonce_format, const unsigned char* pk,
                             int pk_format, const unsigned char* cache, const unsigned char* session) {
    int ok = MUSIG_MAGIC_SESSION(session) & MUSIG_MAGIC_CACHE(cache);
    const int sigma = session[MUSIG_SESSION_PARITY] != 0;
    ge P;
    if (k == 0) {
        ok &= ecdsa_pubkey_load(P, pk, pk_format);
        fe_normalize(P.x); fe_normalize(P.y);
        scalar mu, e;
        musig_keyagg_coef(mu, mid, cache, P);
        sc_set_b32(e, session + MUSIG_SESSION_E, nullptr);
        sc_mul(n, e, mu);
        ge A; musig_point_object(A, cache + MUSIG_CACHE_PK);
        if (fe_is_odd(A.y) != (int)(cache[MUSIG_CACHE_PARITY] & 1)) sc_negate(n, n);
    } else {
        ok &= musig_pubnonce_point(P, nonce, nonce_format, 1);
        sc_set_b32(n, session + MUSIG_SESSION_B, nullptr);
        if (sigma) sc_negate(n, n);
    }
    gej_set_ge(Pj, P);
    return ok;
}

// Returns 1 iff secp256k1_musig_partial_sig_verify would, for item `item`; an item where the reference raises its illegal-argument
// callback (a wrong magic, an all-zero key object) gives 0.  session_of NULL: item i uses cache and session i; an index >= n_sessions
// gives 0.  park: S2K_MUSIG_PARK_WORDS words per lane, word k of lane `lane` at park[k * park_stride + lane].
#define S2K_MUSIG_STAGE_INPUTS \
    const size_t it_ = item + s2k_opaque_zero(); \
    size_t ss_ = session_of ? (size_t)session_of[it_] : it_; \
    const int ss_ok_ = ss_ < n_sessions; ss_ = ss_ok_ ? ss_ : 0; (void)ss_ok_; \
    const unsigned char* const sig = sigs + musig_sig_bytes(sig_format) * it_; (void)sig; \
    const unsigned char* const nonce = nonces + musig_nonce_bytes(nonce_format) * it_; (void)nonce; \
    const unsigned char* const pk = pubkeys + ecdsa_pk_bytes(pk_format) * it_; (void)pk; \
    const unsigned char* const cache = caches + (size_t)MUSIG_CACHE_BYTES * ss_; (void)cache; \
    const unsigned char* const session = sessions + (size_t)MUSIG_SESSION_BYTES * ss_; (void)session; \
    u32* const park = park_base + (lane + s2k_opaque_zero()); (void)park
S2K_HD int musig_verify_lane(const musig_midstates& mid, const unsigned char* sigs, int sig_format, const unsigned char* nonces, int nonce_format,
                             const unsigned char* pubkeys, int pk_format, const unsigned char* caches, const unsigned char* sessions, size_t n_sessions,
                             const u32* session_of, size_t item, int live, const u32* gtab, const lane_mem& lm, u32* park_base, size_t lane, size_t park_stride) {
    int ok = live;
    // ---- T = (-s)*G + sigma*R1: the fixed-base table and one addition
    {
        S2K_MUSIG_STAGE_INPUTS;
        ok &= ss_ok_;
        ok &= MUSIG_MAGIC_SESSION(session) & MUSIG_MAGIC_CACHE(cache) & musig_pubnonce_ok(nonce, nonce_format);
        scalar s; int ov = 0;
        if (sig_format == MUSIG_SIG_OBJECT) { ok &= MUSIG_MAGIC_SIG(sig); sc_set_b32(s, sig + 4, nullptr); }
        else { sc_set_b32(s, sig, &ov); ok &= !ov; }
        sc_negate(s, s);
        if (!ok) sc_set_zero(s);
        gej sG; tweak_gmul_fixed(sG, gtab, s.d);
        ge R1; ok &= musig_pubnonce_point(R1, nonce, nonce_format, 0);           // (after the window loop, as tweak_sum_lane)
        if (session[MUSIG_SESSION_PARITY] != 0) { ge t; ge_neg(t, R1); R1 = t; }
        // s == 0: T = R1; -s*G == R1: the doubling; -s*G == -R1: infinity
        gej T;
        const int f = gej_add_ge(T, sG, R1);
        if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, T); T = d; }
        gej_park(park + S2K_MUSIG_PARK_T * park_stride, park_stride, T);
    }
    // ---- J = e'*P + (sigma*b)*R2
    gej J;
    {
        int joint = 0;
        {
            S2K_MUSIG_STAGE_INPUTS;
            gej Pj, Rj; scalar ne, nb;
            ok &= musig_verify_term(0, Pj, ne, mid, nonce, nonce_format, pk, pk_format, cache, session);
            ok &= musig_verify_term(1, Rj, nb, mid, nonce, nonce_format, pk, pk_format, cache, session);
#if S2K_MUSIG_JOINT
            if (!ok) { sc_set_zero(ne); sc_set_zero(nb); }
            joint = ecmult_lane2(J, Pj, ne, Rj, nb, lm);
#endif
        }
        if (!joint) {
            S2K_MUSIG_STAGE_INPUTS;
            const unsigned char* const nonce_again = nonce; const unsigned char* const pk_again = pk;
            const unsigned char* const cache_again = cache; const unsigned char* const session_again = session;
            auto load = [&](int k, gej& Pj, scalar& n) {
                (void)musig_verify_term(k, Pj, n, mid, nonce_again, nonce_format, pk_again, pk_format, cache_again, session_again);
                if (!ok) sc_set_zero(n);
            };
            ecmult_lane2_calls(J, load, gtab, lm, park + S2K_MUSIG_PARK_FB * park_stride, park_stride);
        }
    }
    // ---- the verdict: J + T is infinity (both infinite counts; J == T is the doubling and fails)
    {
        S2K_MUSIG_STAGE_INPUTS;
        gej T, S;
        gej_unpark(T, park + S2K_MUSIG_PARK_T * park_stride, park_stride);
        gej_add_var(S, J, T);
        ok &= S.inf;
    }
    return ok;
}

// Writes the session of item `item` to sessions_out + 133*item and returns 1 iff secp256k1_musig_nonce_process would; where it returns
// 0 the session is 133 zero bytes (the reference leaves the object untouched).  Nothing is written when !live.  adaptors NULL or
// !HAS_ADAPTOR: no item has an adaptor.  Both to-affine steps are fe_inv_lanes: one inversion per wavefront on the device, so EVERY lane
// of the wavefront must come through here; the first is skipped for the whole launch when HAS_ADAPTOR is 0.
// park: S2K_MUSIG_PARK_R1_WORDS words per lane.
template <int HAS_ADAPTOR>
S2K_HD int musig_process_lane(const musig_midstates& mid, unsigned char* sessions_out, const unsigned char* aggnonces, int nonce_format, const unsigned char* msgs32,
                              const unsigned char* caches, const unsigned char* adaptors, size_t item, int live, const u32* gtab, const lane_mem& lm, u32* park_base,
                              size_t lane, size_t park_stride) {
    int ok = live;
    // ---- the aggregate nonce; with an adaptor R1 += A, to affine.  Then b, and R1 into the parking area
    {
        const size_t it_ = item + s2k_opaque_zero();
        const unsigned char* const nonce = aggnonces + musig_nonce_bytes(nonce_format) * it_;
        const unsigned char* const cache = caches + (size_t)MUSIG_CACHE_BYTES * it_;
        u32* const park = park_base + (lane + s2k_opaque_zero());
        ok &= MUSIG_MAGIC_CACHE(cache);
        ge R[2]; int inf[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (nonce_format == MUSIG_NONCE_OBJECT) {
                inf[k] = musig_all_zero(nonce + 4 + 64 * k, 64);
                musig_point_object(R[k], nonce + 4 + 64 * k);
            } else {
                inf[k] = musig_all_zero(nonce + 33 * k, 33);
                const int parsed = ecdsa_pubkey_load(R[k], nonce + 33 * k, ECDSA_PK_COMPRESSED);
                fe_normalize(R[k].y);
                ok &= parsed | inf[k];
            }
        }
        if (nonce_format == MUSIG_NONCE_OBJECT) ok &= MUSIG_MAGIC_AGGNONCE(nonce);
        if (HAS_ADAPTOR) {
            ge A; ok &= ecdsa_pubkey_load(A, adaptors + 64 * it_, ECDSA_PK_OBJECT);
            gej R1j, S; gej_set_ge(R1j, R[0]); R1j.inf = inf[0];
            const int f = gej_add_ge(S, R1j, A);
            if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, S); S = d; }
            ok &= S.inf | !fe_normalizes_to_zero(S.z);                      // (points off the curve can end at Z = 0 without the flag)
            const int fin = ok & !S.inf;
            fe z = S.z, one, zi; fe_set_int(one, 1);
            fe_cmov(z, one, !fin);
            ok &= fe_inv_lanes(zi, z);
            ge_set_gej_zinv(R[0], S, zi);
            inf[0] = S.inf;
        }
        ge pkp; musig_point_object(pkp, cache + MUSIG_CACHE_PK);
        sha256_stream h; musig_hash_start(h, mid.noncecoef);
        musig_write_ext33(h, R[0], inf[0]); musig_write_ext33(h, R[1], inf[1]);
        unsigned char x32[32]; fe_get_b32(x32, pkp.x);
        sha256_stream_write(h, x32, 32);
        sha256_stream_write(h, msgs32 + 32 * it_, 32);
        scalar b; musig_hash_scalar(b, h);
        if (live) sc_get_b32(sessions_out + (size_t)MUSIG_SESSION_BYTES * it_ + MUSIG_SESSION_B, b);      // (read again below: not held across the multiplication)
#pragma unroll
        for (int i = 0; i < 9; i++) { park[i * park_stride] = R[0].x.n[i]; park[(9 + i) * park_stride] = R[0].y.n[i]; }
        park[18 * park_stride] = (u32)inf[0];
    }
    // ---- F = R1 + b*R2 (an infinite R2 is served by ecmult_lane); infinity becomes G
    gej F;
    {
        const size_t it_ = item + s2k_opaque_zero();
        const unsigned char* const nonce = aggnonces + musig_nonce_bytes(nonce_format) * it_;
        u32* const park = park_base + (lane + s2k_opaque_zero());
        ge R2; int inf2;
        if (nonce_format == MUSIG_NONCE_OBJECT) { inf2 = musig_all_zero(nonce + 68, 64); musig_point_object(R2, nonce + 68); }
        else { inf2 = musig_all_zero(nonce + 33, 33); (void)ecdsa_pubkey_load(R2, nonce + 33, ECDSA_PK_COMPRESSED); }
        scalar nb, zero; sc_set_zero(zero);
        sc_set_b32(nb, sessions_out + (size_t)MUSIG_SESSION_BYTES * (live ? it_ : 0) + MUSIG_SESSION_B, nullptr);
        if (!ok) sc_set_zero(nb);
        gej R2j, T; gej_set_ge(R2j, R2); R2j.inf = inf2 | !ok;
        ecmult_lane(T, R2j, nb, zero, 0, gtab, lm);
        ge R1;
#pragma unroll
        for (int i = 0; i < 9; i++) { R1.x.n[i] = park[i * park_stride]; R1.y.n[i] = park[(9 + i) * park_stride]; }
        const int inf1 = (int)park[18 * park_stride];
        const int f = gej_add_ge(F, T, R1);
        if (f == GEJ_ADD_NEEDS_DOUBLE) { gej d; gej_double(d, F); F = d; }
        if (inf1) F = T;
        ge g; ge_set_generator(g);
        gej Gj; gej_set_ge(Gj, g);
        if (F.inf | !ok) F = Gj;
    }
    // ---- to affine, the challenge, the s part; the session
    {
        const size_t it_ = item + s2k_opaque_zero();
        const unsigned char* const cache = caches + (size_t)MUSIG_CACHE_BYTES * it_;
        unsigned char* const out = sessions_out + (size_t)MUSIG_SESSION_BYTES * it_;
        fe zi; ge a;
        ok &= !fe_normalizes_to_zero(F.z);                                  // (points off the curve can end at Z = 0 without the flag)
        { fe z = F.z, one; fe_set_int(one, 1); fe_cmov(z, one, !ok); ok &= fe_inv_lanes(zi, z); }
        ge_set_gej_zinv(a, F, zi);
        ge pkp; musig_point_object(pkp, cache + MUSIG_CACHE_PK);
        unsigned char fin[32], x32[32];
        fe_get_b32(fin, a.x); fe_get_b32(x32, pkp.x);
        scalar e, sp, tw;
        sha256_stream h; musig_hash_start(h, mid.challenge);
        sha256_stream_write(h, fin, 32); sha256_stream_write(h, x32, 32);
        sha256_stream_write(h, msgs32 + 32 * it_, 32);
        musig_hash_scalar(e, h);
        sc_set_b32(tw, cache + MUSIG_CACHE_TWEAK, nullptr);
        sc_mul(sp, e, tw);                                                  // (a zero tweak gives the 0 the reference sets)
        if (fe_is_odd(pkp.y)) sc_negate(sp, sp);
        if (live) {
            if (ok) {
                out[0] = 0x9d; out[1] = 0xed; out[2] = 0xe9; out[3] = 0x17;
                out[MUSIG_SESSION_PARITY] = (unsigned char)fe_is_odd(a.y);
                for (int i = 0; i < 32; i++) out[MUSIG_SESSION_FIN_NONCE + i] = fin[i];
                unsigned char t[32];                                        // (b is in place already)
                sc_get_b32(t, e); for (int i = 0; i < 32; i++) out[MUSIG_SESSION_E + i] = t[i];
                sc_get_b32(t, sp); for (int i = 0; i < 32; i++) out[MUSIG_SESSION_S_PART + i] = t[i];
            } else {
                for (int i = 0; i < MUSIG_SESSION_BYTES; i++) out[i] = 0;
            }
        }
    }
    return ok;
}
