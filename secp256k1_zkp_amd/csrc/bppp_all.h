// bppp_all.h -- ONE verdict for n Bulletproofs++ norm arguments over ONE generator set, as one multi-scalar multiplication.
// The reference verifies one proof per call (secp256k1_bppp_rangeproof_norm_product_verify, bppp_norm_product_impl.h:425-552, a static);
// the verdict here is the AND of n such calls.
//
// bppp.h folds a proof into one sum  D_p = sum_t sc[p][t] P_{p,t}  that must be the point at infinity (terms in the order of bp_term:
// the generators, G with v_p, the commitment with -1, X_i with -gamma_i, R_i with -(gamma_i^2 - 1)).  Every proof of a deployment uses the
// same generators, so under a random linear combination  sum_p z'_p D_p  the generator terms of ALL proofs collapse:
//
//   generator t < n_gens :  S_t  = sum_p z'_p sc[p][t] mod n          n_gens terms for the whole batch -- scalar arithmetic, no curve arithmetic
//   G                    :  g_sc = sum_p z'_p v_p
//   per proof            :  the commitment with -z'_p, X_{p,i} with -z'_p gamma_{p,i}, R_{p,i} with -z'_p (gamma_{p,i}^2 - 1)
//
// and the n_gens + n (2 n_rounds + 1) points go into one bucket sum (msm_launch).  Coefficients, as schnorr_all.h derives its own (the tree,
// the coefficient and the partial-sum routines ARE schnorr_all.h's, driven with this header's tag midstates):
//
//   T(tag, x) = SHA256(SHA256(tag) | SHA256(tag) | x)
//   gd     = T("S2K/bppp_all/gens", le64(n_gens) | le64(g_len) | gens33)                                  (on the host, once per call)
//   d_p    = T("S2K/bppp_all/item", proof_p | transcript104_p | rho_p | c_vec_p | commit33_p)
//   level 0 = d_0 .. d_{n-1};  node j of the next level = T("S2K/bppp_all/node", nodes 16j .. min(16j + 16, count) - 1)  until one is left
//   seed   = T("S2K/bppp_all/seed", le64(n) | le64(proof_len) | le64(h_len) | gd | root)                  (n = 1: root = d_0)
//   z_0 = 1;  z_p = first 16 bytes, big-endian, of T("S2K/bppp_all/rand", seed | le64(p));  0 -> 1
//   z'_p   = mu z_p mod n,  mu = SHA256("S2K/bppp_all/scale") mod n          (why: sa_scalars in schnorr_all.h; here the commitment's -z_p would be the bare 128-bit value)
// The 104 transcript bytes are hashed as given: bytes of the buffer beyond the fill level change the seed and never the verdict.
//
// Lanes (engine_bppp_all.hip launches them in this order; tests/host_emul/bppp_all_emu.cpp drives them on the host):
//   ba_gen        1 lane / generator      : parse into the sum's 64-byte point record                      } on the side stream, underneath the
//   ba_own_point  1 lane / (proof, own term): the point record, pt_inf where the encoding says infinity     } lanes below: a square root each
//   ba_proof      1 lane / proof          : bp_prologue as it is (sc[p][.] except s_g[1..]), d_p
//   bp_sg_entry   1 lane / (proof, i)     : s_g[i], as in the per-item verifier
//   sa_node       1 lane / parent node    : one launch per level;  ba_seed 1 lane;  ba_coeff 1 lane / proof: z'_p
//   ba_colsum     1 lane / (chunk of BA_CHUNK proofs, column): sum over the chunk of z'_p sc[p][column], columns 0 .. n_gens (the last one is v)
//   ba_colsum_node 1 lane / (parent, column): up to 16 partial sums; the last pass leaves the 32 big-endian bytes the sum reads
//   ba_own_scalar 1 lane / (proof, own term): z'_p sc[p][t]
// Everything is public data; nothing here is constant time.
#pragma once
#include "bppp.h"
#include "schnorr_all.h"

#define BA_CHUNK 32u             /* proofs one lane of the first column-sum pass folds */

// the tree, coefficient and scale slots of schnorr_all.h's struct, with this header's tags
S2K_HD void ba_make_midstates(sa_midstates& m) {
    sa_tag_midstate(m.item, "S2K/bppp_all/item", 17);
    sa_tag_midstate(m.node, "S2K/bppp_all/node", 17);
    sa_tag_midstate(m.seed, "S2K/bppp_all/seed", 17);
    sa_tag_midstate(m.rand, "S2K/bppp_all/rand", 17);
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, (const unsigned char*)"S2K/bppp_all/scale", 18);
    unsigned char b[32]; sha256_stream_finalize(h, b);
    sc_set_b32(m.scale, b, nullptr);
}
S2K_HD void ba_stream_from_midstate(sha256_stream& h, const u32* mid8) {
    for (int k = 0; k < 8; k++) h.s[k] = mid8[k];
    for (int k = 0; k < 16; k++) h.buf[k] = 0;
    h.bytes = 64;
}
S2K_HD void ba_b32_to_words(u32* w8, const unsigned char* b) {
    for (int k = 0; k < 8; k++) w8[k] = s2k_load_be32(b + 4 * k);
}
S2K_HD void ba_write_le64(sha256_stream& h, u64 v) {
    unsigned char b[8];
    for (int k = 0; k < 8; k++) b[k] = (unsigned char)(v >> (8 * k));
    sha256_stream_write(h, b, 8);
}
// gd (8 words): the generator set as the caller serialised it
S2K_HD void ba_gens_digest(u32* gd8, const unsigned char* gens33, size_t n_gens, size_t g_len) {
    u32 mid[8]; sa_tag_midstate(mid, "S2K/bppp_all/gens", 17);
    sha256_stream h; ba_stream_from_midstate(h, mid);
    ba_write_le64(h, (u64)n_gens); ba_write_le64(h, (u64)g_len);
    sha256_stream_write(h, gens33, 33 * n_gens);
    unsigned char d[32]; sha256_stream_finalize(h, d);
    ba_b32_to_words(gd8, d);
}
// d_p (8 words)
S2K_HD void ba_item_digest(u32* digest8, const sa_midstates& mid, const bp_shape& sh, const unsigned char* proof, size_t proof_len, const unsigned char* transcript104,
                           const unsigned char* rho32, const unsigned char* c_vec32, const unsigned char* commit33) {
    sha256_stream h; ba_stream_from_midstate(h, mid.item);
    sha256_stream_write(h, proof, proof_len);
    sha256_stream_write(h, transcript104, 104);
    sha256_stream_write(h, rho32, 32);
    sha256_stream_write(h, c_vec32, 32 * (size_t)sh.h_len);
    sha256_stream_write(h, commit33, 33);
    unsigned char d[32]; sha256_stream_finalize(h, d);
    ba_b32_to_words(digest8, d);
}
// One proof: sc[p][.] (term_sc: n_terms x 8 words; s_g[1..] are left to bp_sg_entry, their factors in sg_factors) and d_p.  Returns what
// bp_prologue returns (0: n or l overflows, or rho is 0); the row of a refused proof is cleared, so that everything behind it reads
// defined scalars (the batch is refused through the flags word whatever the sum says).
S2K_HD int ba_proof(u32* term_sc, u32* sg_factors, u32* digest8, const sa_midstates& mid, const bp_shape& sh, const unsigned char* proof, size_t proof_len,
                    const unsigned char* transcript104, const unsigned char* rho32, const unsigned char* c_vec32, const unsigned char* commit33) {
    const int ok = bp_prologue(term_sc, sh, proof, transcript104, rho32, c_vec32, sg_factors);
    if (!ok) {
        for (u32 k = 0; k < 8 * sh.n_terms; k++) term_sc[k] = 0;
        for (u32 k = 0; k < 8 * BP_MAX_LOG_G; k++) sg_factors[k] = 0;
    }
    ba_item_digest(digest8, mid, sh, proof, proof_len, transcript104, rho32, c_vec32, commit33);
    return ok;
}
S2K_HD void ba_seed(u32* seed8, const sa_midstates& mid, const u32* gd8, const u32* root8, u64 n, u64 proof_len, u64 h_len) {
    u32 st[8], w[16];
    for (int k = 0; k < 8; k++) { st[k] = mid.seed[k]; w[6 + k] = gd8[k]; }
    sa_le64_words(w, n); sa_le64_words(w + 2, proof_len); sa_le64_words(w + 4, h_len);
    w[14] = root8[0]; w[15] = root8[1];
    sha256_compress(st, w);
    for (int k = 0; k < 6; k++) w[k] = root8[2 + k];
    w[6] = 0x80000000u;
    for (int k = 7; k < 15; k++) w[k] = 0;
    w[15] = (64 + 88) * 8;
    sha256_compress(st, w);
    for (int k = 0; k < 8; k++) seed8[k] = st[k];
}
// z'_p = mu z_p (8 little-endian limbs)
S2K_HD void ba_coeff(u32* zp8, const sa_midstates& mid, const u32* seed8, u64 p) {
    scalar z; sa_coeff(z, mid, seed8, p);
    sc_mul(z, z, mid.scale);
    for (int k = 0; k < 8; k++) zp8[k] = z.d[k];
}

// The column sums: an n x (n_gens + 1) matrix of scalars (row p = sc[p][0 .. n_gens], n_terms scalars apart) times the vector z'.
// Pass 0: lane (chunk, column) folds BA_CHUNK proofs; then partial sums with fan-in 16 until one row is left -- at least one such pass,
// which is the one that writes bytes.  counts[0] = chunks, counts[k + 1] = ceil(counts[k] / 16) ... 1; returns the number of entries
// of counts (n = 0: none), i.e. 1 + the number of fan-in passes.
S2K_HD int ba_colsum_plan(size_t* counts, u32* chunk_len, size_t n) {
    *chunk_len = BA_CHUNK;
    if (n == 0) return 0;
    int k = 0;
    size_t c = (n + BA_CHUNK - 1) / BA_CHUNK;
    counts[k++] = c;
    do { c = (c + SA_FANIN - 1) / SA_FANIN; counts[k++] = c; } while (c > 1);
    return k;
}
// rows of 8 x ncols words the passes leave between them (every level but the last, which goes to the sum's arrays)
S2K_HD size_t ba_colsum_rows(size_t n) {
    size_t counts[SA_MAX_LEVELS], t = 0; u32 L;
    const int k = ba_colsum_plan(counts, &L, n);
    for (int i = 0; i + 1 < k; i++) t += counts[i];
    return t;
}
// lane (chunk, col): out8 = sum over p in [p0, p1) of z'_p sc[p][col]
S2K_HD void ba_colsum(u32* out8, const u32* term_sc, const u32* zp, u32 n_terms, u32 col, size_t p0, size_t p1) {
    scalar acc; sc_set_zero(acc);
    for (size_t p = p0; p < p1; p++) {
        scalar a, z;
        for (int k = 0; k < 8; k++) { a.d[k] = term_sc[(p * n_terms + col) * 8 + k]; z.d[k] = zp[8 * p + k]; }
        sc_mul(a, a, z); sc_add(acc, acc, a);
    }
    for (int k = 0; k < 8; k++) out8[k] = acc.d[k];
}
// lane (parent, col): cnt (1..16) rows of in (ncols x 8 words each, starting at the parent's first child); out32 != NULL: the last pass
S2K_HD void ba_colsum_node(u32* out8, unsigned char* out32, const u32* in, u32 ncols, u32 col, u32 cnt) {
    scalar acc;
    for (int k = 0; k < 8; k++) acc.d[k] = in[8 * col + k];
    for (u32 j = 1; j < cnt; j++) { scalar t; for (int k = 0; k < 8; k++) t.d[k] = in[((size_t)j * ncols + col) * 8 + k]; sc_add(acc, acc, t); }
    if (out32) sc_get_b32(out32, acc);
    else for (int k = 0; k < 8; k++) out8[k] = acc.d[k];
}
// an affine point (or infinity) as the sum reads it: x | y big-endian, and the pt_inf byte
S2K_HD void ba_store_point(unsigned char* xy64, unsigned char* inf1, ge& p, int inf) {
    if (inf) { for (int k = 0; k < 64; k++) xy64[k] = 0; *inf1 = 1; return; }
    fe_normalize(p.x); fe_normalize(p.y);
    fe_get_b32(xy64, p.x); fe_get_b32(xy64 + 32, p.y);
    *inf1 = 0;
}
S2K_HD int ba_gen(unsigned char* xy64, unsigned char* inf1, const unsigned char* gen33) {
    ge p; const int ok = bp_parse33(p, gen33);
    ba_store_point(xy64, inf1, p, !ok);
    return ok;
}
// the point of own term j of a proof (0: the commitment, 1 + 2i: X_i, 2 + 2i: R_i), exactly as bp_term reads it: returns whether it parsed; a
// point that did not parse goes in as infinity (the flags word refuses the batch).  Needs nothing but the inputs.
S2K_HD int ba_own_point(unsigned char* xy64, unsigned char* inf1, u32 j, const unsigned char* proof, const unsigned char* commit33) {
    int ok = 1, inf = 0;
    ge p;
    if (j == 0) {
        u32 nz = 0; for (int i = 0; i < 33; i++) nz |= commit33[i];
        if (nz) { ok = bp_parse33(p, commit33); inf = !ok; } else inf = 1;
    } else {
        const u32 r = j - 1, i = r >> 1, idx = r & 1;
        ok = bp_parse_one_of_points(p, inf, proof + 65 * i, (int)idx);
        inf |= !ok;
    }
    ba_store_point(xy64, inf1, p, inf);
    return ok;
}
// its scalar: sc32 = z'_p sc[p][n_gens + 1 + j]
S2K_HD void ba_own_scalar(unsigned char* sc32, const bp_shape& sh, u32 j, const u32* term_sc, const u32* zp8) {
    scalar a, z;
    for (int k = 0; k < 8; k++) { a.d[k] = term_sc[8 * (sh.n_gens + 1 + j) + k]; z.d[k] = zp8[k]; }
    sc_mul(a, a, z);
    sc_get_b32(sc32, a);
}
