// whitelist.h -- whitelist-signature verification (secp256k1_whitelist_verify, src/modules/whitelist/main_impl.h:99-129) in two lane
// routines:
//   wl_key_lane   one lane per (item, key) pair : ring key  K_j = online_j + t_j (offline_j + sub),  t_j = SHA256(ser33(offline_j + sub))
//                                                 (secp256k1_whitelist_compute_keys_and_message, whitelist_impl.h:89-125, :10-50)
//   wl_ring_lane  one lane per item             : msg32 = SHA256(ser33(sub) | ser33(offline_0) | ser33(online_0) | ...), the signature's
//                                                 structure, then ONE Borromean ring (ring index 0) of n_keys positions
//                                                 (secp256k1_borromean_verify, src/modules/rangeproof/borromean_impl.h:53-104)
// A serialised signature is  n_keys (1 byte) | e0 (32) | s_0 .. s_{n-1} (32 each)  (secp256k1_whitelist_signature_parse :135-151).
// Keys are 64-byte secp256k1_pubkey objects (ecdsa_pubkey_load, ECDSA_PK_OBJECT).  An all-zero key object, where the reference calls
// its illegal-argument callback and then reads an unset point, makes the item 0 here.
// Both routines are flag-and-select as ecdsa.h: no lane leaves in front of ecmult_lane or fe_inv_lanes (one to-affine inversion per
// wavefront), dead lanes ride along with zero scalars and hand in z = 1.
#pragma once
#include "ecdsa.h"
#include "rangeproof.h"      // gej_store28_h / gej_load28_h, rp_words_to_scalar, rp_hash_e0

#define WL_MAX_KEYS 255u
#define WL_KEY_WORDS RP_GEJ_WORDS      /* a ring key in the workspace: 28 words, the layout of gej_store28_h */

S2K_HD u64 wl_sig_bytes(u64 n_keys) { return 1 + 32 * (n_keys + 1); }
// does this item run at all?  (list length, signature length; the n_keys byte itself is read by wl_ring_lane)
S2K_HD int wl_item_planned(u64 n_keys, u64 siglen) { return (n_keys <= WL_MAX_KEYS) & (siglen == wl_sig_bytes(n_keys)); }

// ser33 of a normalised affine point as the hash wants it: prefix 2 | odd(y), x as 8 big-endian words
S2K_HD void wl_ser33(u32& prefix, u32 xb[8], const ge& a) {
    u32 xw[8]; fe_to_words(xw, a.x);
#pragma unroll
    for (int i = 0; i < 8; i++) xb[i] = xw[7 - i];
    prefix = 2u | (u32)fe_is_odd(a.y);
}
S2K_HD void wl_add_ge(gej& r, const gej& a, const ge& b) {                 // secp256k1_gej_add_ge_var: a == b is a doubling
    const int f = gej_add_ge(r, a, b);
    if (f == GEJ_ADD_NEEDS_DOUBLE) { gej t; gej_double(t, r); r = t; }
}

// ---- SHA-256 of a byte stream without a dynamically indexed buffer ---------------------------------------------------------------------
// The block is a 512-bit shift register: a byte goes in at the bottom, so after 64 of them w[0..15] is the block in message order
// whatever the alignment of the pieces was.  ~35 instructions per byte, every index static: nothing goes to scratch
// (sha256_stream's buf[pos >> 2] would).
struct wl_sha { u32 s[8]; u32 w[16]; u64 bytes; };
S2K_HD void wl_sha_init(wl_sha& c) {
    sha256_init(c.s);
#pragma unroll
    for (int i = 0; i < 16; i++) c.w[i] = 0;
    c.bytes = 0;
}
S2K_HD void wl_sha_put(wl_sha& c, u32 byte) {
#pragma unroll
    for (int i = 0; i < 15; i++) c.w[i] = (c.w[i] << 8) | (c.w[i + 1] >> 24);
    c.w[15] = (c.w[15] << 8) | byte;
    c.bytes++;
    if ((c.bytes & 63) == 0) {
        u32 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = c.w[i];
        sha256_compress(c.s, w);
    }
}
// the 33 bytes prefix | x
S2K_HD void wl_sha_put33(wl_sha& c, u32 prefix, const u32 xb[8]) {
    u32 r[9];
    r[0] = (prefix << 24) | (xb[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; i++) r[i] = (xb[i - 1] << 24) | (xb[i] >> 8);
    r[8] = xb[7] << 24;
#pragma unroll 1
    for (int k = 0; k < 33; k++) {
        wl_sha_put(c, r[0] >> 24);
#pragma unroll
        for (int i = 0; i < 8; i++) r[i] = (r[i] << 8) | (r[i + 1] >> 24);
        r[8] <<= 8;
    }
}
S2K_HD void wl_sha_finalize(wl_sha& c, u32 out[8]) {
    const u64 bits = c.bytes << 3;
    u32 pad = 0x80u;
#pragma unroll 1
    do { wl_sha_put(c, pad); pad = 0; } while ((c.bytes & 63) != 56);
    u32 w[16];                                                  // the 56 bytes of the last block are the register's bottom 14 words
#pragma unroll
    for (int i = 0; i < 14; i++) w[i] = c.w[i + 2];
    w[14] = (u32)(bits >> 32); w[15] = (u32)bits;
    sha256_compress(c.s, w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = c.s[i];
}

// SHA256(ser33): one block
S2K_HD void wl_hash33(u32 out[8], u32 prefix, const u32 xb[8]) {
    u32 st[8], w[16];
    sha256_init(st);
    w[0] = (prefix << 24) | (xb[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; i++) w[i] = (xb[i - 1] << 24) | (xb[i] >> 8);
    w[8] = (xb[7] << 24) | 0x00800000u;
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = 33 * 8;
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = st[i];
}
// last == 0:  H(ser33 | m | ring 0 | epos)  -- rp_hash_step(out, prefix, xb, m, 0, epos), secp256k1_borromean_hash with a 33-byte e
// last == 1:  SHA256(ser33 | m)             -- what e0 is compared with (borromean_impl.h:95-103 for one ring)
// The two messages share their first block (ser33 and 31 bytes of m); the second block is chosen by selects, so that a wavefront
// whose lanes end their rings at different positions does not walk the compression twice.
S2K_HD void wl_hash_step(u32 out[8], u32 prefix, const u32 xb[8], const u32 m[8], u32 epos, int last) {
    u32 st[8], w[16];
    sha256_init(st);
    w[0] = (prefix << 24) | (xb[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; i++) w[i] = (xb[i - 1] << 24) | (xb[i] >> 8);
    w[8] = (xb[7] << 24) | (m[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; i++) w[8 + i] = (m[i - 1] << 24) | (m[i] >> 8);
    sha256_compress(st, w);
    w[0] = (m[7] << 24) | (last ? 0x00800000u : 0u);
    w[1] = last ? 0u : (epos >> 8);
    w[2] = last ? 0u : ((epos << 24) | 0x00800000u);
#pragma unroll
    for (int i = 3; i < 15; i++) w[i] = 0;
    w[15] = last ? 65u * 8u : 73u * 8u;
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = st[i];
}

// ---- ring key of one (item, key) pair ---------------------------------------------------------------------------------------------------
// K = online + t (offline + sub) as a Jacobian record at key28 (written iff live).  whitelist_impl.h:117-120: the return value of
// secp256k1_whitelist_tweak_pubkey is ignored, so where it fails -- offline + sub is infinity, or t overflows / is 0, "mathematically
// impossible" -- the sum stays untweaked:  K = (offline + sub) + online.  A key object that does not load gives an infinity record,
// which makes the item 0 (borromean_impl.h:77).  An off-curve object with y == 0 doubles to Z == 0: taken as infinity (the reference
// is undefined for off-curve objects; this keeps the wavefront's shared inversion alive for the other lanes).
// Returns whether the three key objects loaded and the wave inverse did not report a zero (0: the record is infinity).
S2K_HD int wl_key_lane(u32* key28, const unsigned char* online64, const unsigned char* offline64, const unsigned char* sub64, int live,
                       const u32* gtab, const lane_mem& lm) {
    int ok = live;
    gej A;
    {
        ge off, sub;
        ok &= ecdsa_pubkey_load(off, offline64, ECDSA_PK_OBJECT);
        ok &= ecdsa_pubkey_load(sub, sub64, ECDSA_PK_OBJECT);
        gej offj; gej_set_ge(offj, off);
        wl_add_ge(A, offj, sub);
    }
    A.inf |= fe_normalizes_to_zero(A.z);
    fe z = A.z, one, zi;
    fe_set_int(one, 1);
    fe_cmov(z, one, !ok | A.inf);
    ok &= fe_inv_lanes(zi, z);                                   // 0: clears the item's verdict through the infinity record
    ge a; ge_set_gej_zinv(a, A, zi);                             // offline + sub, affine (meaningless where A.inf or !ok)
    scalar t, zero; int ov;
    {
        u32 prefix, xb[8], h[8];
        wl_ser33(prefix, xb, a);
        wl_hash33(h, prefix, xb);
        rp_words_to_scalar(t, ov, h);
    }
    const int tweak = ok & !A.inf & !ov & !sc_is_zero(t);
    sc_set_zero(zero);
    if (!tweak) sc_set_zero(t);                                  // nothing to multiply: ride along
    gej Aj; gej_set_ge(Aj, a); Aj.inf = A.inf | !ok;
    if (live) gej_store28_h(key28, Aj);                           // nothing but flags and pointers stays live across ecmult_lane
    gej T;
    ecmult_lane(T, Aj, t, zero, 0, gtab, lm);
    if (!tweak) { if (live) gej_load28_h(T, key28); else gej_set_infinity(T); }
    ge on; gej K;
    ok &= ecdsa_pubkey_load(on, online64, ECDSA_PK_OBJECT);
    wl_add_ge(K, T, on);
    K.inf |= fe_normalizes_to_zero(K.z);
    if (!ok) gej_set_infinity(K);
    if (live) gej_store28_h(key28, K);
    return ok;
}

// ---- one item: message hash, structure, the ring -----------------------------------------------------------------------------------------
// keys28: the item's n_keys ring-key records (wl_key_lane); msg8: 8 words of this item's own scratch, where msg32 lies while the ring
// runs (re-read after every multiplication instead of being kept in registers).  n_keys is the LIST's length: the reference's
// `sig->n_keys != n_keys` is the first byte of the signature against it.  Returns the verdict.
// The ring loop runs to the wavefront's largest n_keys; a lane past its own ring, or dead, rides along (rp_ring's convention).
S2K_HD int wl_ring_lane(const unsigned char* sig, u64 siglen, const u32* keys28, const unsigned char* online64, const unsigned char* offline64,
                        u64 n_keys, const unsigned char* sub64, u32* msg8, int live, const u32* gtab, const lane_mem& lm) {
    int ok = live & wl_item_planned(n_keys, siglen);
    if (ok) ok &= (u64)sig[0] == n_keys;                          // never touch the bytes of an item that failed its structural checks
    const u32 nk = ok ? (u32)n_keys : 0u;
    if (ok) {
        for (u32 j = 0; j < nk; j++) {                            // main_impl.h:115-121
            scalar s; int ov;
            sc_set_b32(s, sig + 33 + 32 * (size_t)j, &ov);
            ok &= !ov & !sc_is_zero(s);
        }
    }
    if (ok) {                                                     // whitelist_impl.h:97-122
        wl_sha c; wl_sha_init(c);
#pragma unroll 1
        for (u32 k = 0; k < 2 * nk + 1; k++) {
            const unsigned char* p = k == 0 ? sub64 : ((k & 1) ? offline64 : online64) + 64 * (size_t)((k - 1) >> 1);
            ge P; u32 prefix, xb[8];
            ok &= ecdsa_pubkey_load(P, p, ECDSA_PK_OBJECT);
            wl_ser33(prefix, xb, P);
            wl_sha_put33(c, prefix, xb);
        }
        u32 m[8]; wl_sha_finalize(c, m);
#pragma unroll
        for (int i = 0; i < 8; i++) msg8[i] = m[i];
    }
    u32 e[8];
    {
        u32 m[8], e0[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { m[i] = ok ? msg8[i] : 0u; e0[i] = ok ? s2k_load_be32(sig + 1 + 4 * i) : 0u; }
        rp_hash_e0(e, e0, m, 0);
        if (ok && nk == 0) {                                      // the empty ring: e0 == SHA256(msg32)
            u32 st[8], w[16];
            sha256_init(st);
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = m[i];
            w[8] = 0x80000000u;
#pragma unroll
            for (int i = 9; i < 15; i++) w[i] = 0;
            w[15] = 32 * 8;
            sha256_compress(st, w);
#pragma unroll
            for (int i = 0; i < 8; i++) ok &= st[i] == e0[i];
        }
    }
#pragma unroll 1
    for (u32 j = 0; S2K_WAVE_ANY(j < nk); j++) {
        const int in_ring = j < nk;
        const int step_live = ok & in_ring;
        scalar ens, s; int ov_e, ov_s = 0;
        rp_words_to_scalar(ens, ov_e, e);
        sc_set_zero(s);
        gej pub; gej_set_infinity(pub);
        if (step_live) { sc_set_b32(s, sig + 33 + 32 * (size_t)j, &ov_s); gej_load28_h(pub, keys28 + WL_KEY_WORDS * (size_t)j); }
        int good = step_live & !ov_e & !ov_s & !sc_is_zero(s) & !sc_is_zero(ens) & !pub.inf;
        if (!good) { sc_set_zero(ens); sc_set_zero(s); }          // dead lanes ride along with empty work
        gej R;
        ecmult_lane(R, pub, ens, s, 1, gtab, lm);
        good &= !R.inf;
        fe z = R.z, one, zi;
        fe_set_int(one, 1);
        fe_cmov(z, one, !good);
        good &= fe_inv_lanes(zi, z);                              // 0: some lane handed in z == 0, every inverse of the wavefront is meaningless
        ge a; ge_set_gej_zinv(a, R, zi);
        u32 prefix, xb[8], m[8];
        wl_ser33(prefix, xb, a);
        if (in_ring) ok &= good;
        const int last = j + 1 == nk;
#pragma unroll
        for (int i = 0; i < 8; i++) m[i] = step_live ? msg8[i] : 0u;
        wl_hash_step(e, prefix, xb, m, j + 1, last);
        if (step_live & last) {
#pragma unroll
            for (int i = 0; i < 8; i++) ok &= e[i] == s2k_load_be32(sig + 1 + 4 * i);
        }
    }
    return ok;
}
