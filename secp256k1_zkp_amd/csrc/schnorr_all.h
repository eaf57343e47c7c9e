// schnorr_all.h -- ONE verdict for n BIP-340 signatures: the batch verification the BIP describes ("Batch Verification", the
// equation  (s_1 + a_2 s_2 + ...) G = R_1 + a_2 R_2 + ... + e_1 P_1 + (a_2 e_2) P_2 + ...), as one multi-scalar multiplication.
// The reference has no such call: the verdict is the AND of n secp256k1_schnorrsig_verify (src/modules/schnorrsig/main_impl.h:215-261).
//
//   accept  <=>  -(sum a_i s_i) G + sum a_i R_i + sum (a_i e_i) P_i  is the point at infinity
//   R_i = lift_x(r_i) (even y),  e_i = H_BIP0340/challenge(r_i | x(P_i) | m_i) mod n  (:106-120),  a_0 = 1, a_i 128 random bits
//
// The coefficients are derived from the batch itself, and -- unlike the half-aggregate randomizers z_i, which hash the whole PREFIX
// up to item i and are therefore one Merkle-Damgard chain (halfagg.h) -- from a hash TREE, whose depth is all that is serial:
//
//   T(tag, x) = SHA256(SHA256(tag) | SHA256(tag) | x)
//   d_i    = T("S2K/schnorr_all/item", sig_i | x32_i | m_i)          x32_i: the key's 32 serialised bytes (format 1: the object's x, big-endian)
//   level 0 = d_0 .. d_{n-1};  node j of the next level = T("S2K/schnorr_all/node", nodes 16j .. min(16j + 16, count) - 1)  until one is left
//   seed   = T("S2K/schnorr_all/seed", le64(n) | le64(msglen) | root)                                     (n = 1: root = d_0)
//   a_i    = first 16 bytes, big-endian, of T("S2K/schnorr_all/rand", seed | le64(i));  0 -> 1;  a_0 = 1
//
// Lanes (engine_schnorr_all.hip launches them in this order; tests/host_emul/schnorr_all_emu.cpp drives them on the host):
//   sa_item      1 lane / signature   : ha_points (the lift and the key), s_i < n, d_i, e_i
//   sa_node      1 lane / parent node : up to 16 children, 8 full blocks + the padding; one launch per level
//   sa_seed      1 lane
//   sa_scalars   1 lane / signature   : a_i, the MSM scalars mu a_i and mu a_i e_i and the term mu a_i s_i (mu: a fixed public factor, see there)
//   sa_sum_node  1 lane / parent      : up to 16 terms added mod n; the last level negates
// Everything is public data; nothing here is constant time.
#pragma once
#include "halfagg_batch.h"

#define SA_FANIN 16u
#define SA_MAX_LEVELS 20         /* 16^16 = 2^64: a size_t count is one node after at most 16 levels */

struct sa_midstates { u32 item[8], node[8], seed[8], rand[8]; scalar scale; };

// SHA256 state after the 64-byte prefix SHA256(tag) x 2
S2K_HD void sa_tag_midstate(u32 s[8], const char* tag, size_t len) {
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)tag, len);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);
    for (int i = 0; i < 8; i++) s[i] = g.s[i];
}
S2K_HD void sa_make_midstates(sa_midstates& m) {
    sa_tag_midstate(m.item, "S2K/schnorr_all/item", 20);
    sa_tag_midstate(m.node, "S2K/schnorr_all/node", 20);
    sa_tag_midstate(m.seed, "S2K/schnorr_all/seed", 20);
    sa_tag_midstate(m.rand, "S2K/schnorr_all/rand", 20);
    // mu = SHA256("S2K/schnorr_all/scale") mod n: see sa_scalars
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)"S2K/schnorr_all/scale", 21);
    unsigned char b[32]; sha256_stream_finalize(h, b);
    sc_set_b32(m.scale, b, nullptr);
}

// The level plan: counts[0] = n, counts[k + 1] = ceil(counts[k] / 16) down to one node; returns the number of levels (n = 0: none).
// The node array holds the levels back to back, so the root is its last entry.
S2K_HD int sa_level_plan(size_t* counts, size_t n) {
    if (n == 0) return 0;
    int levels = 0;
    size_t c = n;
    for (;;) {
        counts[levels++] = c;
        if (c == 1) break;
        c = (c + SA_FANIN - 1) / SA_FANIN;
    }
    return levels;
}
// entries of the node array (all levels), and of the array of the scalar sum's partial sums (every level after the terms themselves,
// at least one: a single term still goes through one pass, which negates it)
S2K_HD size_t sa_node_count(size_t n) {
    size_t counts[SA_MAX_LEVELS], t = 0;
    const int levels = sa_level_plan(counts, n);
    for (int k = 0; k < levels; k++) t += counts[k];
    return t;
}
S2K_HD size_t sa_sum_count(size_t n) { return n <= 1 ? n : sa_node_count(n) - n; }

// big-endian word q of  msg | 0x80 | 0 0 0 ...
S2K_HD u32 sa_msg_word(const unsigned char* msg, size_t msglen, size_t q) {
    const size_t b = 4 * q;
    if (b + 4 <= msglen) return ha_be32(msg + b);
    u32 w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t j = b + k;
        const u32 v = j < msglen ? (u32)msg[j] : (j == msglen ? 0x80u : 0u);
        w |= v << (24 - 8 * k);
    }
    return w;
}
// st has taken `done` bytes (a multiple of 64); absorbs  head (hw words, 0 or 8) | msg, pads and finalises
S2K_HD void sa_tail(u32 st[8], const u32* head, int hw, const unsigned char* msg, size_t msglen, u64 done) {
    const u64 bits = (done + 4 * (u64)hw + msglen) * 8;
    const size_t nb = (4 * (size_t)hw + msglen + 9 + 63) / 64;
    for (size_t b = 0; b < nb; b++) {
        u32 w[16];
#pragma unroll
        for (int t = 0; t < 16; t++) w[t] = (b == 0 && t < hw) ? head[t & 7] : sa_msg_word(msg, msglen, 16 * b + t - hw);
        if (b + 1 == nb) { w[14] = (u32)(bits >> 32); w[15] = (u32)bits; }
        sha256_compress(st, w);
    }
}
S2K_HD void sa_words_to_b32(unsigned char* out, const u32* w) {
#pragma unroll
    for (int k = 0; k < 8; k++) s2k_store_be32(out + 4 * k, w[k]);
}

// One signature: the MSM's points R_i, P_i (pt128) and x(P_i) as ha_points leaves them, the item digest d_i (8 words) and the challenge
// e_i (32 bytes, reduced).  Returns 0 if r_i >= p, r_i is not an x coordinate, the key does not parse (an all-zero object included) or
// s_i >= n: the conditions of schnorr_verify_lane.  d_i hashes the key as the CALLER serialised it (hab_key8), e_i hashes x(P_i) as
// schnorr_verify_lane does; for every key that parses the two are the same bytes.
S2K_HD int sa_item(unsigned char* pt128, u32* digest8, unsigned char* e32, const sa_midstates& mid, const schnorr_midstate& bip340, const unsigned char* sig64,
                   const unsigned char* msg, size_t msglen, const unsigned char* pk, int pk_format) {
    unsigned char pkx32[32];
    int ok = ha_points(pt128, pkx32, sig64, pk, pk_format);
    { scalar s; int ov; sc_set_b32(s, sig64 + 32, &ov); ok &= !ov; }
    u32 r8[8], s8[8], x8[8];
    hab_load8(r8, sig64); hab_load8(s8, sig64 + 32);
    {   // d_i: tag | r_i s_i | x32_i m_i ...
        u32 st[8], w[16];
        for (int k = 0; k < 8; k++) { st[k] = mid.item[k]; w[k] = r8[k]; w[8 + k] = s8[k]; }
        sha256_compress(st, w);
        hab_key8(x8, pk, pk_format);
        sa_tail(st, x8, 8, msg, msglen, 128);
        for (int k = 0; k < 8; k++) digest8[k] = st[k];
    }
    {   // e_i: tag | r_i x(P_i) | m_i ...
        u32 st[8], w[16];
        for (int k = 0; k < 8; k++) { st[k] = bip340.s[k]; w[k] = r8[k]; w[8 + k] = s2k_load_be32(pkx32 + 4 * k); }
        sha256_compress(st, w);
        sa_tail(st, x8, 0, msg, msglen, 128);
        unsigned char buf[32]; sa_words_to_b32(buf, st);
        scalar e; sc_set_b32(e, buf, nullptr);
        sc_get_b32(e32, e);
    }
    return ok;
}
// one parent node: cnt (1..16) children of 8 words each
S2K_HD void sa_node(u32* out8, const sa_midstates& mid, const u32* child, u32 cnt) {
    u32 st[8], w[16];
    for (int k = 0; k < 8; k++) st[k] = mid.node[k];
    const u64 bits = (u64)(64 + 32 * cnt) * 8;
    for (u32 j = 0; j + 1 < cnt; j += 2) {
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = child[8 * j + k];
        sha256_compress(st, w);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 0;
    if (cnt & 1) {
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = child[8 * (cnt - 1) + k];
        w[8] = 0x80000000u;
    } else w[0] = 0x80000000u;
    w[14] = (u32)(bits >> 32); w[15] = (u32)bits;
    sha256_compress(st, w);
    for (int k = 0; k < 8; k++) out8[k] = st[k];
}
// le64(v) as the two big-endian words a block holds
S2K_HD void sa_le64_words(u32* w2, u64 v) { w2[0] = __builtin_bswap32((u32)v); w2[1] = __builtin_bswap32((u32)(v >> 32)); }
S2K_HD void sa_seed(u32* seed8, const sa_midstates& mid, const u32* root8, u64 n, u64 msglen) {
    u32 st[8], w[16];
    for (int k = 0; k < 8; k++) { st[k] = mid.seed[k]; w[4 + k] = root8[k]; }
    sa_le64_words(w, n); sa_le64_words(w + 2, msglen);
    w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = (64 + 48) * 8;
    sha256_compress(st, w);
    for (int k = 0; k < 8; k++) seed8[k] = st[k];
}
S2K_HD void sa_coeff(scalar& a, const sa_midstates& mid, const u32* seed8, u64 i) {
    if (i == 0) { sc_set_int(a, 1); return; }
    u32 st[8], w[16];
    for (int k = 0; k < 8; k++) { st[k] = mid.rand[k]; w[k] = seed8[k]; }
    sa_le64_words(w + 8, i);
    w[10] = 0x80000000u; w[11] = 0; w[12] = 0; w[13] = 0; w[14] = 0; w[15] = (64 + 40) * 8;
    sha256_compress(st, w);
    sc_set_zero(a);
    a.d[3] = st[0]; a.d[2] = st[1]; a.d[1] = st[2]; a.d[0] = st[3];
    if (sc_is_zero(a)) sc_set_int(a, 1);
}
// sc64: in, e_i in its second half (sa_item); out, mu a_i | mu a_i e_i.  t32 = mu a_i s_i (s_i reduced: an s_i >= n has already failed the batch).
// Every scalar of the sum carries the same public factor mu != 0, which changes nothing about when the sum is the point at infinity
// (mu X = O  <=>  X = O in a group of prime order): the statement checked is the one with the a_i.  It is there for the bucket sums'
// sake.  The MSM splits every scalar by the curve's endomorphism (k = k1 + k2 lambda), and for k < 2^128 the second half is one of a
// handful of constants: half of a batch's a_i would meet in ONE bucket of every window, overflow its region and send the whole sum
// down the exact, bucket-free path (measured at 2^21 terms: 73.7 ms that way, 3.1 ms with mu).  mu a_i mod n splits into two halves that
// look uniform.
S2K_HD void sa_scalars(unsigned char* sc64, unsigned char* t32, const sa_midstates& mid, const u32* seed8, const unsigned char* s32, u64 i) {
    scalar a, e, s;
    sa_coeff(a, mid, seed8, i);
    sc_mul(a, a, mid.scale);
    sc_set_b32(e, sc64 + 32, nullptr);
    sc_set_b32(s, s32, nullptr);
    sc_mul(e, e, a); sc_mul(s, s, a);
    sc_get_b32(sc64, a); sc_get_b32(sc64 + 32, e);
    sc_get_b32(t32, s);
}
// one parent of the scalar sum: cnt (1..16) terms of 32 bytes; negate: this is the last level, leave -(sum)
S2K_HD void sa_sum_node(unsigned char* out32, const unsigned char* in32, u32 cnt, int negate) {
    scalar acc; sc_set_b32(acc, in32, nullptr);
    for (u32 j = 1; j < cnt; j++) { scalar t; sc_set_b32(t, in32 + 32 * j, nullptr); sc_add(acc, acc, t); }
    if (negate) sc_negate(acc, acc);
    sc_get_b32(out32, acc);
}
