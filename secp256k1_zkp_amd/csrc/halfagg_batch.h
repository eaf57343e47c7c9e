// halfagg_batch.h -- MANY half-aggregated BIP-340 signatures per call: batch verification (secp256k1_schnorrsig_aggverify,
// src/modules/schnorrsig_halfagg/main_impl.h:108-198) and batch (incremental) aggregation (secp256k1_schnorrsig_inc_aggregate, :19-102).
//
// One aggregate alone is a serial SHA-256 chain (z_i hashes the whole prefix r_0|x(P_0)|m_0|...|r_i|x(P_i)|m_i) in front of one
// multi-scalar multiplication: latency from end to end (halfagg.h).  The chain is serial only WITHIN an aggregate, so a batch runs
//   hab_chain_lane   1 lane / aggregate : the full 64-byte blocks of the aggregate's stream, schedule and rounds in registers, the
//                                         state after every block stored (32 bytes a block) -- exactly what ha_scalars reads
//   ha_points        1 lane / signature : as for one aggregate, into the point array of K sums side by side
//   ha_scalars       1 lane / signature : z_i (one more compression on a copy of the state), e_i, the two MSM scalars; local index, so
//                                         that z_0 = 1 per aggregate
//   ha_gscalar       1 lane / aggregate : -s_k
//   (K sums)                            : s2k_ecmult_multi_many's launch chain over 2 n_k terms per aggregate, g_sc = -s_k
// and aggregation is the same chain followed by  t_i = z_i s_i  per signature and  s = s_old + sum t_i  per aggregate.
// Layout: aggregate k owns items [item_off[k], item_off[k+1]) of the key and message arrays; its chain states start at block
// (3 item_off[k]) >> 1 of ONE state array -- floor is superadditive, floor(3a/2) + floor(3n/2) <= floor(3(a+n)/2), so the ranges of
// neighbours never overlap whatever the parities.  An aggregate whose length is not 32 (n_k + 1) bytes is refused (main_impl.h:122-125)
// and owns no MSM terms; neither does one with more than `max_terms` terms, which goes through the single-aggregate path instead.
#pragma once
#include "halfagg.h"
#include <algorithm>
#include <vector>

// the aggregate of item i: the last k with off[k] <= i (empty aggregates own no item).  off[0] = 0 <= i < off[n_aggs].
S2K_HD size_t hab_segment(const u64* off, size_t n_aggs, u64 i) {
    size_t lo = 0, hi = n_aggs;
    while (hi - lo > 1) { const size_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
S2K_HD size_t hab_state_slot(u64 first_item) { return (size_t)((3 * first_item) >> 1); }
// main_impl.h:122-125
S2K_HD int hab_len_ok(u64 n, u64 len) { return (len / 32) != 0 && (len / 32) - 1 == n && (len % 32) == 0; }
// verification: 0 refused by length, 1 a sum of the batch, 2 over the limit (the single-aggregate path)
S2K_HD int hab_kind(const u64* item_off, const u64* agg_off, size_t k, u64 max_terms) {
    const u64 n = item_off[k + 1] - item_off[k];
    if (!hab_len_ok(n, agg_off[k + 1] - agg_off[k])) return 0;
    return 2 * n > max_terms ? 2 : 1;
}

// eight big-endian words of a 32-byte unit
S2K_HD void hab_load8(u32* w, const unsigned char* p) {
    if ((((size_t)p) & 3u) == 0u) {
        const unsigned char* q = (const unsigned char*)__builtin_assume_aligned(p, 4);
#pragma unroll
        for (int t = 0; t < 8; t++) { u32 x; __builtin_memcpy(&x, q + 4 * t, 4); w[t] = __builtin_bswap32(x); }
    } else {
#pragma unroll
        for (int t = 0; t < 8; t++) w[t] = ha_be32(p + 4 * t);
    }
}
// x(P) as hashed, straight from the input: format 0 the 32 bytes are x; format 1 the object's first 32 bytes, least significant first
// (a key that turns out invalid makes the verdict 0 whatever was hashed)
S2K_HD void hab_key8(u32* w, const unsigned char* pk, int pk_format) {
    if (!pk_format) { hab_load8(w, pk); return; }
#pragma unroll
    for (int t = 0; t < 8; t++) { const unsigned char* q = pk + 28 - 4 * t; w[t] = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24); }
}
S2K_HD void hab_block(u32 st[8], u32 w[16], u32* states, size_t& b) {
    sha256_compress(st, w);
#pragma unroll
    for (int t = 0; t < 8; t++) states[8 * b + t] = st[t];
    b++;
}
// The chain of ONE aggregate: r32 its r_j (32 bytes apart), pks / msgs32 its first key / message; (3 n) >> 1 states are written.
// Two items are three blocks: r|x(P), m|r', x(P')|m'; an odd last item leaves its m as a half block, which z finalises (ha_scalars).
S2K_HD void hab_chain_lane(u32* states, const unsigned char* r32, const unsigned char* pks, int pk_format, const unsigned char* msgs32, size_t n) {
    u32 st[8], w[16];
    ha_tag_midstate(st);
    const size_t pkb = pk_format ? 64 : 32;
    size_t b = 0;
    for (size_t i = 0; i + 1 < n; i += 2) {
        hab_load8(w, r32 + 32 * i); hab_key8(w + 8, pks + pkb * i, pk_format); hab_block(st, w, states, b);
        hab_load8(w, msgs32 + 32 * i); hab_load8(w + 8, r32 + 32 * (i + 1)); hab_block(st, w, states, b);
        hab_key8(w, pks + pkb * (i + 1), pk_format); hab_load8(w + 8, msgs32 + 32 * (i + 1)); hab_block(st, w, states, b);
    }
    if (n & 1) { hab_load8(w, r32 + 32 * (n - 1)); hab_key8(w + 8, pks + pkb * (n - 1), pk_format); hab_block(st, w, states, b); }
}

// ---- verification: the per-item and per-aggregate lanes over the batch's arrays -------------------------------------------------------
struct hab_verify_view {
    const u64* item_off; const u64* agg_off; const u64* moff;   // n_aggs + 1 entries each; moff: first MSM term of every aggregate
    size_t n_aggs;
    const unsigned char* pks; int pk_format; const unsigned char* msgs32; const unsigned char* aggsigs;
    unsigned char* pts; unsigned char* sc; unsigned char* g_sc; unsigned char* pkx; u32* states; u32* fail;
};
S2K_HD void hab_points_item(const hab_verify_view& v, u64 i) {
    const size_t k = hab_segment(v.item_off, v.n_aggs, i);
    if (v.moff[k + 1] == v.moff[k]) return;                        // refused by length, or over the limit: no terms
    const u64 j = i - v.item_off[k], slot = (v.moff[k] >> 1) + j;
    if (!ha_points(v.pts + 128 * slot, v.pkx + 32 * i, v.aggsigs + v.agg_off[k] + 32 * j, v.pks + (v.pk_format ? 64 : 32) * i, v.pk_format)) v.fail[k] = 1u;
}
S2K_HD void hab_scalars_item(const hab_verify_view& v, const schnorr_midstate& bip340, u64 i) {
    const size_t k = hab_segment(v.item_off, v.n_aggs, i);
    if (v.moff[k + 1] == v.moff[k]) return;
    const u64 first = v.item_off[k], j = i - first, slot = (v.moff[k] >> 1) + j;
    // an aggregate the points pass has failed (a launch earlier) is decided: zero scalars, which the sums skip, keep its points -- some of
    // them not on the curve -- out of the curve arithmetic
    if (v.fail[k]) { unsigned char* o = v.sc + 64 * slot; for (int t = 0; t < 64; t++) o[t] = 0; return; }
    ha_scalars(v.sc + 64 * slot, v.states + 8 * hab_state_slot(first), bip340, v.aggsigs + v.agg_off[k], v.pkx + 32 * first, v.msgs32 + 32 * first, (size_t)j);
}
S2K_HD void hab_gscalar_agg(const hab_verify_view& v, size_t k) {
    unsigned char* g = v.g_sc + 32 * k;
    const u64 n = v.item_off[k + 1] - v.item_off[k];
    if (v.moff[k + 1] == v.moff[k] && (n || !hab_len_ok(0, v.agg_off[k + 1] - v.agg_off[k]))) { for (int t = 0; t < 32; t++) g[t] = 0; return; }
    if (!ha_gscalar(g, v.aggsigs + v.agg_off[k] + 32 * n)) v.fail[k] = 1u;
}
// 1 / 0, or -1: the single-aggregate path writes this verdict
S2K_HD int hab_verdict(const u64* item_off, const u64* agg_off, size_t k, u64 max_terms, u32 fail, int r_inf) {
    const int kind = hab_kind(item_off, agg_off, k, max_terms);
    if (kind == 2) return -1;
    return kind == 1 && !fail && r_inf;
}

// ---- aggregation ------------------------------------------------------------------------------------------------------------------------
// Aggregate k: n_k items, of which the first nb_k = (in_off[k+1] - in_off[k]) / 32 - 1 are already in aggsigs_in (r_0..r_{nb-1} | s_old at
// byte in_off[k]; in_off NULL: nb_k = 0 everywhere, the plain aggregation) and the rest are signatures new_off[k] .. of new_sigs64.
// The output aggregate k is at byte 32 (item_off[k] + k).
struct hab_agg_view {
    const u64* item_off; const u64* in_off; const u64* new_off; size_t n_aggs;
    const unsigned char* pks; int pk_format; const unsigned char* msgs32; const unsigned char* aggsigs_in; const unsigned char* new_sigs64;
    unsigned char* out; unsigned char* t32; u32* states; u32* fail;
};
S2K_HD u64 hab_n_before(const hab_agg_view& v, size_t k) { return v.in_off ? (v.in_off[k + 1] - v.in_off[k]) / 32 - 1 : 0; }
S2K_HD unsigned char* hab_out_of(const hab_agg_view& v, size_t k) { return v.out + 32 * (v.item_off[k] + k); }
// r_j into the output (the chain reads it there), and the key check: format 0 as secp256k1_xonly_pubkey_parse (x < p and on the curve),
// format 1 the all-zero-x object that xonly_pubkey_serialize refuses (main_impl.h:47, :70)
S2K_HD void hab_gather_item(const hab_agg_view& v, u64 i) {
    const size_t k = hab_segment(v.item_off, v.n_aggs, i);
    const u64 j = i - v.item_off[k], nb = hab_n_before(v, k);
    const unsigned char* r = j < nb ? v.aggsigs_in + v.in_off[k] + 32 * j : v.new_sigs64 + 64 * (v.new_off[k] + (j - nb));
    unsigned char* o = hab_out_of(v, k) + 32 * j;
    for (int t = 0; t < 32; t++) o[t] = r[t];
    int ok;
    if (v.pk_format == 0) { fe x; ge P; ok = fe_set_b32_limit(x, v.pks + 32 * i); ok &= ge_set_xo(P, x, 0); }
    else { fe x; fe_set_le32(x, v.pks + 64 * i); ok = !fe_normalizes_to_zero(x); }
    if (!ok) v.fail[k] = 1u;
}
// z_j of an aggregate from its chain states (j = 0: 1, main_impl.h:88-90)
S2K_HD void hab_z(scalar& z, const u32* states, const unsigned char* msgs32, size_t j) {
    if (j == 0) { sc_set_int(z, 1); return; }
    const size_t full = (3 * (j + 1)) >> 1;
    u32 st[8], w[16];
    for (int t = 0; t < 8; t++) st[t] = states[(full - 1) * 8 + t];
    for (int t = 0; t < 16; t++) w[t] = 0;
    int pos = 0;
    if ((j + 1) & 1) { hab_load8(w, msgs32 + 32 * j); pos = 8; }
    w[pos] = 0x80000000u;
    const u64 bits = (u64)(64 + 96 * (j + 1)) * 8;
    w[14] = (u32)(bits >> 32); w[15] = (u32)bits;
    sha256_compress(st, w);
    unsigned char out[32];
    for (int t = 0; t < 8; t++) s2k_store_be32(out + 4 * t, st[t]);
    sc_set_b32(z, out, nullptr);
}
// t_i = z_j s_i for a new item (s_i reduced, not refused: main_impl.h:89); a refused aggregate gets its r_j zeroed again
S2K_HD void hab_term_item(const hab_agg_view& v, u64 i) {
    const size_t k = hab_segment(v.item_off, v.n_aggs, i);
    const u64 first = v.item_off[k], j = i - first, nb = hab_n_before(v, k);
    if (v.fail[k]) { unsigned char* o = hab_out_of(v, k) + 32 * j; for (int t = 0; t < 32; t++) o[t] = 0; return; }
    if (j < nb) return;
    scalar z, s;
    hab_z(z, v.states + 8 * hab_state_slot(first), v.msgs32 + 32 * first, (size_t)j);
    sc_set_b32(s, v.new_sigs64 + 64 * (v.new_off[k] + (j - nb)) + 32, nullptr);
    sc_mul(s, s, z);
    sc_get_b32(v.t32 + 32 * i, s);
}
// s = s_old + sum t_i behind the r's (s_old without an overflow check and only when nb > 0: main_impl.h:60-61); returns the verdict
S2K_HD int hab_sum_agg(const hab_agg_view& v, size_t k) {
    const u64 first = v.item_off[k], n = v.item_off[k + 1] - first, nb = hab_n_before(v, k);
    unsigned char* o = hab_out_of(v, k) + 32 * n;
    if (v.fail[k]) { for (int t = 0; t < 32; t++) o[t] = 0; return 0; }
    scalar s; sc_set_zero(s);
    if (nb > 0) sc_set_b32(s, v.aggsigs_in + v.in_off[k] + 32 * nb, nullptr);
    for (u64 j = nb; j < n; j++) { scalar t; sc_set_b32(t, v.t32 + 32 * (first + j), nullptr); sc_add(s, s, t); }
    sc_get_b32(o, s);
    return 1;
}

// ---- host plans (the launcher and the host emulation share them) -------------------------------------------------------------------------
// Lane -> aggregate of the chain kernel: the listed aggregates by descending item count (a counting sort over the host offsets), so that
// the lanes of a wavefront, which runs as long as its longest lane, have chains of like length.  Aggregates without a full block are left out.
static inline std::vector<u32> hab_chain_order(const u64* item_off, const std::vector<u32>& which) {
    u64 nmax = 0;
    for (u32 k : which) nmax = std::max(nmax, (u64)(item_off[k + 1] - item_off[k]));
    std::vector<size_t> start((size_t)nmax + 2, 0);
    for (u32 k : which) { const u64 n = item_off[k + 1] - item_off[k]; if (n) start[(size_t)(nmax - n) + 1]++; }
    for (size_t q = 1; q < start.size(); q++) start[q] += start[q - 1];
    std::vector<u32> perm(start.back());
    for (u32 k : which) { const u64 n = item_off[k + 1] - item_off[k]; if (n) perm[start[(size_t)(nmax - n)]++] = k; }
    return perm;
}
struct hab_verify_plan {
    std::vector<u64> moff;       // n_aggs + 1: 2 n_k terms for a sum of the batch, none for a refused or an over-limit aggregate
    std::vector<u32> perm;       // chain lanes
    std::vector<u32> large;      // over the limit, length right: the single-aggregate path, one by one
};
static inline hab_verify_plan hab_plan_verify(const u64* item_off, const u64* agg_off, size_t n_aggs, u64 max_terms) {
    hab_verify_plan p; p.moff.assign(n_aggs + 1, 0);
    std::vector<u32> batch;
    for (size_t k = 0; k < n_aggs; k++) {
        const int kind = hab_kind(item_off, agg_off, k, max_terms);
        p.moff[k + 1] = p.moff[k] + (kind == 1 ? 2 * (item_off[k + 1] - item_off[k]) : 0);
        if (kind == 1) batch.push_back((u32)k); else if (kind == 2) p.large.push_back((u32)k);
    }
    p.perm = hab_chain_order(item_off, batch);
    return p;
}
