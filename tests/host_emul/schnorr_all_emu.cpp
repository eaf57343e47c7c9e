// tests/host_emul/schnorr_all_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/schnorr_all.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp (included as it is, so this library
// carries its own copy of the generator table and is loaded next to libs2k_hostemu.so).  The lane functions run in the order
// engine_schnorr_all.hip launches them, one "lane" after the other, over scratch arrays of exactly the carved sizes: the items, one pass
// per tree level over the level plan, the seed, the scalars, one pass per level of the scalar sum.  The (2n+1)-term sum is then evaluated
// with the host group law, one double multiplication per term; where the verdict is 0 and results are asked for, the per-item lane
// (schnorr_verify_lane) says which items failed, as the host entry point does.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/schnorr_all.h"

namespace {
struct sa_run {
    std::vector<unsigned char> pts, sc, t, sums;
    std::vector<u32> nodes;
    u32 seed[8];
    const unsigned char* g32;
    int ok;
};
// everything in front of the sum; with_scalars 0 stops behind the seed
void sa_front(sa_run& r, const unsigned char* sigs, const unsigned char* msgs, size_t msglen, const unsigned char* pks, int pk_format, size_t n, int with_scalars) {
    sa_midstates mid; sa_make_midstates(mid);
    schnorr_midstate bip; schnorr_tag_midstate(bip);
    size_t counts[SA_MAX_LEVELS];
    const int levels = sa_level_plan(counts, n);
    r.pts.assign(128 * n, 0xEE); r.sc.assign(64 * n, 0xEE); r.t.assign(32 * n, 0xEE); r.sums.assign(32 * sa_sum_count(n), 0xEE);
    r.nodes.assign(8 * sa_node_count(n), 0xEEEEEEEEu);
    r.ok = 1;
    for (size_t i = 0; i < n; i++)
        r.ok &= sa_item(r.pts.data() + 128 * i, r.nodes.data() + 8 * i, r.sc.data() + 64 * i + 32, mid, bip, sigs + 64 * i, msgs + msglen * i, msglen,
                        pks + (pk_format ? 64 : 32) * i, pk_format);
    u32* level = r.nodes.data();
    for (int k = 0; k + 1 < levels; k++) {
        u32* next = level + 8 * counts[k];
        for (size_t j = 0; j < counts[k + 1]; j++) {
            const size_t left = counts[k] - SA_FANIN * j;
            sa_node(next + 8 * j, mid, level + 8 * SA_FANIN * j, left < SA_FANIN ? (u32)left : SA_FANIN);
        }
        level = next;
    }
    sa_seed(r.seed, mid, level, n, msglen);
    if (!with_scalars) return;
    for (size_t i = 0; i < n; i++) sa_scalars(r.sc.data() + 64 * i, r.t.data() + 32 * i, mid, r.seed, sigs + 64 * i + 32, i);
    const unsigned char* in = r.t.data(); unsigned char* out = r.sums.data();
    size_t cnt = n;
    do {
        const size_t cnt_out = (cnt + SA_FANIN - 1) / SA_FANIN;
        for (size_t j = 0; j < cnt_out; j++) {
            const size_t left = cnt - SA_FANIN * j;
            sa_sum_node(out + 32 * j, in + 32 * SA_FANIN * j, left < SA_FANIN ? (u32)left : SA_FANIN, cnt_out == 1);
        }
        in = out; out += 32 * cnt_out; cnt = cnt_out;
    } while (cnt > 1);
    r.g32 = in;
}
}

extern "C" {
// the level plan: counts of every level into counts[] (at most `cap`), returns the number of levels; totals[0] nodes, totals[1] partial sums
int emu_schnorr_all_plan(uint64_t* counts, uint64_t* totals, size_t n, int cap) {
    size_t c[SA_MAX_LEVELS];
    const int levels = sa_level_plan(c, n);
    for (int k = 0; k < levels && k < cap; k++) counts[k] = c[k];
    totals[0] = sa_node_count(n); totals[1] = sa_sum_count(n);
    return levels;
}
// seed (32 bytes) and the n coefficients (16 bytes each, big-endian) of a batch; no curve sum
int emu_schnorr_all_seed(unsigned char* seed32, unsigned char* coeffs16, const unsigned char* sigs, const unsigned char* msgs, size_t msglen,
                         const unsigned char* pks, int pk_format, size_t n) {
    if (!seed32 || pk_format < 0 || pk_format > 1 || ((!sigs || !pks || (!msgs && msglen)) && n)) return 0;
    memset(seed32, 0, 32);
    if (n == 0) return 1;
    sa_run r; sa_front(r, sigs, msgs, msglen, pks, pk_format, n, 0);
    sa_words_to_b32(seed32, r.seed);
    if (coeffs16) {
        sa_midstates mid; sa_make_midstates(mid);
        for (size_t i = 0; i < n; i++) {
            scalar a; sa_coeff(a, mid, r.seed, i);
            unsigned char b[32]; sc_get_b32(b, a);
            for (int k = 0; k < 16; k++) if (b[k]) return -1;          // a coefficient has 128 bits
            memcpy(coeffs16 + 16 * i, b + 16, 16);
        }
    }
    return 1;
}
// returns 0 where the engine returns S2K_STATUS_ILLEGAL_ARGUMENT
int emu_schnorr_verify_all(int32_t* verdict, int32_t* results, unsigned char* seed32, const unsigned char* sigs, const unsigned char* msgs, size_t msglen,
                           const unsigned char* pks, int pk_format, size_t n) {
    if (!verdict || pk_format < 0 || pk_format > 1 || ((!sigs || !pks || (!msgs && msglen)) && n)) return 0;
    *verdict = 0;
    if (results) for (size_t i = 0; i < n; i++) results[i] = 0;
    if (seed32) memset(seed32, 0, 32);
    if (n == 0) { *verdict = 1; return 1; }
    sa_run r; sa_front(r, sigs, msgs, msglen, pks, pk_format, n, 1);
    if (seed32) sa_words_to_b32(seed32, r.seed);
    // g * G + sum sc_j * pt_j over the 2n points R_0, P_0, R_1, P_1, ...  (a batch the items pass has refused is decided: its points need
    // not be on the curve, and the device's sum over them cannot change the verdict either)
    int inf = 0;
    if (r.ok) {
        gej acc; gej_set_infinity(acc);
        for (size_t j = 0; j <= 2 * n; j++) {
            gej A, R; scalar k, g; gej_set_infinity(A); sc_set_zero(k); sc_set_zero(g);
            if (j < 2 * n) { ge a; ge_from_b64(a, r.pts.data() + 64 * j); fe_norm_weak(a.x); fe_norm_weak(a.y); gej_set_ge(A, a); sc_set_b32(k, r.sc.data() + 32 * j, 0); }
            else sc_set_b32(g, r.g32, 0);
            u32 dig[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig};
            ecmult_lane(R, A, k, g, 1, gtab_host(), lm);
            gej s; gej_add_var(s, acc, R); acc = s;
        }
        inf = acc.inf;
    }
    *verdict = r.ok && inf;
    if (results) {
        schnorr_midstate mid; schnorr_tag_midstate(mid);
        for (size_t i = 0; i < n; i++)
            results[i] = *verdict ? 1 : schnorr_verify_lane(mid, sigs + 64 * i, msgs + msglen * i, msglen, pks + (pk_format ? 64 : 32) * i, pk_format, 1, gtab_host(), g_lm);
    }
    return 1;
}
}
