// tests/host_emul/bppp_all_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/bppp_all.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp (included as it is, so this library
// carries its own copy of the generator table and is loaded next to libs2k_hostemu.so).  The lane functions run in the order
// engine_bppp_all.hip launches them, one "lane" after the other, over scratch arrays of exactly the carved sizes: the generators and
// the proofs' own points, the proofs, the s_g entries, one pass per tree level over the level plan, the seed, the coefficients, the column sums over the column-sum
// plan, the own terms' scalars.  The sum over the n_gens + n (2 n_rounds + 1) points and G is then evaluated with the host group law, one double
// multiplication per term; where the verdict is 0 and results are asked for, the per-item verifier (emu_bppp_verify) says which proofs
// failed, as the host entry point does.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/bppp_all.h"

namespace {
struct ba_args {
    const unsigned char* proofs; size_t proof_len; const unsigned char* trs; const unsigned char* rho; const unsigned char* gens33; size_t n_gens, g_len;
    const unsigned char* cvec; size_t h_len; const unsigned char* commits; size_t n;
};
struct ba_run {
    std::vector<u32> term_sc, fac, nodes, zp, part;
    std::vector<unsigned char> pts, inf, sc, gsc;
    u32 seed[8];
    int ok;
};
int ba_args_ok(const ba_args& a) { return !((!a.proofs || !a.trs || !a.rho || !a.gens33 || !a.cvec || !a.commits) && a.n); }
// the item digests, the tree and the seed: hashes only (the proofs need not be proofs)
void ba_hashes(ba_run& r, const sa_midstates& mid, const bp_shape& sh, const ba_args& a, int digests) {
    const size_t n = a.n;
    size_t counts[SA_MAX_LEVELS];
    const int levels = sa_level_plan(counts, n);
    if (digests) {
        r.nodes.assign(8 * sa_node_count(n), 0xEEEEEEEEu);
        for (size_t p = 0; p < n; p++)
            ba_item_digest(r.nodes.data() + 8 * p, mid, sh, a.proofs + p * a.proof_len, a.proof_len, a.trs + 104 * p, a.rho + 32 * p, a.cvec + 32 * sh.h_len * p, a.commits + 33 * p);
    }
    u32* level = r.nodes.data();
    for (int k = 0; k + 1 < levels; k++) {
        u32* next = level + 8 * counts[k];
        for (size_t j = 0; j < counts[k + 1]; j++) {
            const size_t left = counts[k] - SA_FANIN * j;
            sa_node(next + 8 * j, mid, level + 8 * SA_FANIN * j, left < SA_FANIN ? (u32)left : SA_FANIN);
        }
        level = next;
    }
    u32 gd[8]; ba_gens_digest(gd, a.gens33, sh.n_gens, sh.g_len);
    ba_seed(r.seed, mid, gd, level, n, a.proof_len, sh.h_len);
    r.zp.assign(8 * n, 0xEEEEEEEEu);
    for (size_t p = 0; p < n; p++) ba_coeff(r.zp.data() + 8 * p, mid, r.seed, p);
}
// everything in front of the sum
void ba_front(ba_run& r, const bp_shape& sh, const ba_args& a) {
    sa_midstates mid; ba_make_midstates(mid);
    const size_t n = a.n, own = 2 * (size_t)sh.n_rounds + 1, M = sh.n_gens + n * own, ncols = sh.n_gens + 1;
    r.ok = 1;
    r.pts.assign(64 * M, 0xEE); r.inf.assign(M, 0xEE); r.sc.assign(32 * M, 0xEE); r.gsc.assign(32, 0xEE);
    r.term_sc.assign(n * sh.n_terms * 8, 0xEEEEEEEEu); r.fac.assign(n * 8 * BP_MAX_LOG_G, 0xEEEEEEEEu);
    r.nodes.assign(8 * sa_node_count(n), 0xEEEEEEEEu);
    for (size_t i = 0; i < sh.n_gens; i++) r.ok &= ba_gen(r.pts.data() + 64 * i, r.inf.data() + i, a.gens33 + 33 * i);
    for (size_t p = 0; p < n; p++)
        for (u32 j = 0; j < own; j++) { const size_t o = sh.n_gens + p * own + j; r.ok &= ba_own_point(r.pts.data() + 64 * o, r.inf.data() + o, j, a.proofs + p * a.proof_len, a.commits + 33 * p); }
    std::vector<int> proof_ok(n);
    for (size_t p = 0; p < n; p++) {
        proof_ok[p] = ba_proof(r.term_sc.data() + p * sh.n_terms * 8, r.fac.data() + p * 8 * BP_MAX_LOG_G, r.nodes.data() + 8 * p, mid, sh, a.proofs + p * a.proof_len, a.proof_len,
                               a.trs + 104 * p, a.rho + 32 * p, a.cvec + 32 * sh.h_len * p, a.commits + 33 * p);
        r.ok &= proof_ok[p];
    }
    for (size_t p = 0; p < n; p++)
        for (u32 i = 1; i < sh.g_len; i++) if (proof_ok[p]) bp_sg_entry(r.term_sc.data() + p * sh.n_terms * 8, r.fac.data() + p * 8 * BP_MAX_LOG_G, sh, i);
    ba_hashes(r, mid, sh, a, 0);
    size_t cc[SA_MAX_LEVELS]; u32 L;
    const int cp = ba_colsum_plan(cc, &L, n);
    r.part.assign(ba_colsum_rows(n) * ncols * 8, 0xEEEEEEEEu);
    for (size_t ch = 0; ch < cc[0]; ch++)
        for (u32 col = 0; col < ncols; col++) {
            const size_t p0 = ch * L, p1 = std::min(p0 + L, n);
            ba_colsum(r.part.data() + (ch * ncols + col) * 8, r.term_sc.data(), r.zp.data(), sh.n_terms, col, p0, p1);
        }
    const u32* in = r.part.data();
    for (int k = 0; k + 1 < cp; k++) {
        const int last = (k + 2 == cp);
        u32* out = const_cast<u32*>(in) + cc[k] * ncols * 8;
        for (size_t j = 0; j < cc[k + 1]; j++)
            for (u32 col = 0; col < ncols; col++) {
                const size_t left = cc[k] - SA_FANIN * j;
                ba_colsum_node(last ? nullptr : out + (j * ncols + col) * 8, last ? (col + 1 < ncols ? r.sc.data() + 32 * col : r.gsc.data()) : nullptr,
                               in + SA_FANIN * j * ncols * 8, (u32)ncols, col, left < SA_FANIN ? (u32)left : SA_FANIN);
            }
        in = out;
    }
    for (size_t p = 0; p < n; p++)
        for (u32 j = 0; j < own; j++) {
            const size_t o = sh.n_gens + p * own + j;
            ba_own_scalar(r.sc.data() + 32 * o, sh, j, r.term_sc.data() + p * sh.n_terms * 8, r.zp.data() + 8 * p);
        }
}
void words_to_b32(unsigned char* out, const u32* limbs8) { scalar s; for (int k = 0; k < 8; k++) s.d[k] = limbs8[k]; sc_get_b32(out, s); }
}

extern "C" {
unsigned emu_bppp_all_chunk(void) { return BA_CHUNK; }
// the level plan of the hash tree into counts[], the column-sum plan into ccounts[] (at most `cap` each); out4 = {levels, entries of ccounts, chunk length,
// rows of partial sums}; totals[0] nodes of the tree
int emu_bppp_all_plan(uint64_t* counts, uint64_t* ccounts, uint64_t* out4, uint64_t* totals, size_t n, int cap) {
    size_t c[SA_MAX_LEVELS], cc[SA_MAX_LEVELS]; u32 L;
    const int levels = sa_level_plan(c, n), cp = ba_colsum_plan(cc, &L, n);
    for (int k = 0; k < levels && k < cap; k++) counts[k] = c[k];
    for (int k = 0; k < cp && k < cap; k++) ccounts[k] = cc[k];
    out4[0] = (uint64_t)levels; out4[1] = (uint64_t)cp; out4[2] = L; out4[3] = ba_colsum_rows(n);
    totals[0] = sa_node_count(n);
    return levels;
}
// seed (32 bytes), the n coefficients z_p (16 bytes each, big-endian) and z'_p (32 bytes each) of a batch; hashes only
int emu_bppp_all_seed(unsigned char* seed32, unsigned char* coeffs16, unsigned char* zp32, const unsigned char* proofs, size_t proof_len, const unsigned char* trs,
                      const unsigned char* rho, const unsigned char* gens33, size_t n_gens, size_t g_len, const unsigned char* cvec, size_t h_len,
                      const unsigned char* commits, size_t n) {
    const ba_args a{proofs, proof_len, trs, rho, gens33, n_gens, g_len, cvec, h_len, commits, n};
    if (!seed32 || !ba_args_ok(a)) return 0;
    memset(seed32, 0, 32);
    if (n == 0) return 1;
    bp_shape sh;
    if (!bp_make_shape(sh, g_len, h_len, n_gens, proof_len)) return 1;
    sa_midstates mid; ba_make_midstates(mid);
    ba_run r; ba_hashes(r, mid, sh, a, 1);
    sa_words_to_b32(seed32, r.seed);
    for (size_t p = 0; p < n; p++) {
        if (coeffs16) {
            scalar z; sa_coeff(z, mid, r.seed, p);
            unsigned char b[32]; sc_get_b32(b, z);
            for (int k = 0; k < 16; k++) if (b[k]) return -1;          // a coefficient has 128 bits
            memcpy(coeffs16 + 16 * p, b + 16, 16);
        }
        if (zp32) words_to_b32(zp32 + 32 * p, r.zp.data() + 8 * p);
    }
    return 1;
}
// what the sum is fed: sc[p][t] (n x n_terms x 32 bytes), z'_p (n x 32), S_t (n_gens x 32), g_sc (32), the own-term scalars (n x (2 n_rounds + 1) x 32),
// the pt_inf bytes (n_gens + n (2 n_rounds + 1)); returns the flags' verdict (every proof passed the prologue and every point parsed), -1 for a refused shape
int emu_bppp_all_scalars(unsigned char* sc_out, unsigned char* zp_out, unsigned char* S_out, unsigned char* gsc_out, unsigned char* own_out, unsigned char* inf_out,
                         const unsigned char* proofs, size_t proof_len, const unsigned char* trs, const unsigned char* rho, const unsigned char* gens33, size_t n_gens,
                         size_t g_len, const unsigned char* cvec, size_t h_len, const unsigned char* commits, size_t n) {
    const ba_args a{proofs, proof_len, trs, rho, gens33, n_gens, g_len, cvec, h_len, commits, n};
    bp_shape sh;
    if (!n || !ba_args_ok(a) || !bp_make_shape(sh, g_len, h_len, n_gens, proof_len) || sh.log_g > BP_MAX_LOG_G) return -1;
    ba_run r; ba_front(r, sh, a);
    const size_t own = 2 * (size_t)sh.n_rounds + 1;
    for (size_t i = 0; i < n * sh.n_terms; i++) words_to_b32(sc_out + 32 * i, r.term_sc.data() + 8 * i);
    for (size_t p = 0; p < n; p++) words_to_b32(zp_out + 32 * p, r.zp.data() + 8 * p);
    memcpy(S_out, r.sc.data(), 32 * n_gens); memcpy(gsc_out, r.gsc.data(), 32);
    memcpy(own_out, r.sc.data() + 32 * n_gens, 32 * n * own);
    memcpy(inf_out, r.inf.data(), n_gens + n * own);
    return r.ok;
}
// returns 0 where the engine returns S2K_STATUS_ILLEGAL_ARGUMENT (max_terms: the limit of one sum, 0 = the engine's default), -1 where it fails otherwise
int emu_bppp_verify_all(int32_t* verdict, int32_t* results, unsigned char* seed32, const unsigned char* proofs, size_t proof_len, const unsigned char* trs,
                        const unsigned char* rho, const unsigned char* gens33, size_t n_gens, size_t g_len, const unsigned char* cvec, size_t h_len,
                        const unsigned char* commits, size_t n, size_t max_terms) {
    const ba_args a{proofs, proof_len, trs, rho, gens33, n_gens, g_len, cvec, h_len, commits, n};
    if (!verdict || !ba_args_ok(a)) return 0;
    *verdict = 0;
    bp_shape sh;
    const int shape_ok = n ? bp_make_shape(sh, g_len, h_len, n_gens, proof_len) : 0;
    if (shape_ok && sh.log_g > BP_MAX_LOG_G) return -1;
    if (shape_ok) {
        const size_t cap = max_terms ? max_terms : ((size_t(1) << 32) - 1) / 18 - 1, own = 2 * (size_t)sh.n_rounds + 1;
        if (sh.n_gens >= cap || n > (cap - 1 - sh.n_gens) / own) return 0;
    }
    if (results) for (size_t i = 0; i < n; i++) results[i] = 0;
    if (seed32) memset(seed32, 0, 32);
    if (n == 0) { *verdict = 1; return 1; }
    if (!shape_ok) return 1;
    ba_run r; ba_front(r, sh, a);
    if (seed32) sa_words_to_b32(seed32, r.seed);
    int inf = 0;
    if (r.ok) {
        const size_t M = r.inf.size();
        gej acc; gej_set_infinity(acc);
        for (size_t j = 0; j <= M; j++) {
            gej A, R; scalar k, g; gej_set_infinity(A); sc_set_zero(k); sc_set_zero(g);
            if (j < M) {
                if (!r.inf[j]) { ge pa; ge_from_b64(pa, r.pts.data() + 64 * j); fe_norm_weak(pa.x); fe_norm_weak(pa.y); gej_set_ge(A, pa); }
                sc_set_b32(k, r.sc.data() + 32 * j, 0);
            } else sc_set_b32(g, r.gsc.data(), 0);
            u32 dig[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig};
            ecmult_lane(R, A, k, g, 1, gtab_host(), lm);
            gej s; gej_add_var(s, acc, R); acc = s;
        }
        inf = acc.inf;
    }
    *verdict = r.ok && inf;
    if (results)
        for (size_t p = 0; p < n; p++)
            results[p] = *verdict ? 1 : emu_bppp_verify(proofs + p * proof_len, proof_len, trs + 104 * p, rho + 32 * p, gens33, n_gens, g_len, cvec + 32 * h_len * p, h_len, commits + 33 * p);
    return 1;
}
}
