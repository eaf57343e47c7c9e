// tests/host_emul/halfagg_batch_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/halfagg_batch.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp (included as it is, so this library
// carries its own copy of the generator table and is loaded next to libs2k_hostemu.so).  The three batch forms drive the lane functions in
// the order engine_halfagg_batch.hip launches them, one "lane" after the other, over scratch arrays of exactly the carved sizes: the same
// plan (hab_plan_verify: MSM offsets, the lane -> aggregate permutation of the chain kernel, the over-limit list), the same state slots,
// the same binary search.  The K sums are emu_msm per aggregate; an over-limit aggregate goes through emu_halfagg_verify, the emulation
// of the single-aggregate path.  max_terms is the launcher's MM_MAX_TERMS (8 192), a parameter here so that a test can set it to 8.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/halfagg_batch.h"

static int offsets_ok(const uint64_t* off, size_t K) {
    if (!off || off[0] != 0) return 0;
    for (size_t k = 0; k < K; k++) if (off[k + 1] < off[k]) return 0;
    return 1;
}

extern "C" {
// returns 0 where the engine returns S2K_STATUS_ILLEGAL_ARGUMENT
int emu_halfagg_verify_batch(int32_t* results, const unsigned char* pks, int pk_format, const unsigned char* msgs32, const uint64_t* item_off,
                             const unsigned char* aggsigs, const uint64_t* agg_off, size_t K, uint64_t max_terms) {
    if (K == 0) return 1;
    if (!results || !aggsigs || pk_format < 0 || pk_format > 1 || !offsets_ok(item_off, K) || !offsets_ok(agg_off, K)) return 0;
    if (item_off[K] && (!pks || !msgs32)) return 0;
    for (size_t k = 0; k < K; k++) results[k] = 0;
    const hab_verify_plan p = hab_plan_verify(item_off, agg_off, K, max_terms);
    const size_t N = (size_t)item_off[K], NT = (size_t)(p.moff[K] >> 1);
    std::vector<unsigned char> pts(128 * NT + 1), sc(64 * NT + 1), g(32 * K, 0xEE), pkx(32 * N + 1);
    std::vector<u32> states(8 * (hab_state_slot(N) + 1), 0xEEEEEEEEu), fail(K, 0);
    const hab_verify_view v{item_off, agg_off, p.moff.data(), K, pks, pk_format, msgs32, aggsigs, pts.data(), sc.data(), g.data(), pkx.data(), states.data(), fail.data()};
    for (size_t lane = 0; lane < p.perm.size(); lane++) {
        const size_t k = p.perm[lane]; const uint64_t first = item_off[k];
        hab_chain_lane(states.data() + 8 * hab_state_slot(first), aggsigs + agg_off[k], pks + (pk_format ? 64 : 32) * first, pk_format, msgs32 + 32 * first,
                       (size_t)(item_off[k + 1] - first));
    }
    for (size_t i = 0; i < N; i++) hab_points_item(v, i);
    schnorr_midstate mid; schnorr_tag_midstate(mid);
    for (size_t i = 0; i < N; i++) hab_scalars_item(v, mid, i);
    for (size_t k = 0; k < K; k++) hab_gscalar_agg(v, k);
    for (size_t k = 0; k < K; k++) {
        unsigned char r64[64];
        const size_t slot = (size_t)(p.moff[k] >> 1), nt = (size_t)(p.moff[k + 1] - p.moff[k]);
        const int inf = emu_msm(r64, g.data() + 32 * k, sc.data() + 64 * slot, pts.data() + 128 * slot, nullptr, nt, 0);
        if (inf < 0) return -1;
        const int r = hab_verdict(item_off, agg_off, k, max_terms, fail[k], inf);
        if (r >= 0) results[k] = r;
    }
    for (u32 k : p.large) {
        const size_t first = (size_t)item_off[k];
        results[k] = emu_halfagg_verify(pks + (pk_format ? 64 : 32) * first, pk_format, msgs32 + 32 * first, (size_t)(item_off[k + 1] - first), aggsigs + agg_off[k],
                                        (size_t)(agg_off[k + 1] - agg_off[k]));
    }
    return 1;
}
// how the plan splits a batch: [0] sums of the batch with terms, [1] chain lanes, [2] over-limit aggregates
void emu_halfagg_plan(uint64_t* out3, const uint64_t* item_off, const uint64_t* agg_off, size_t K, uint64_t max_terms) {
    const hab_verify_plan p = hab_plan_verify(item_off, agg_off, K, max_terms);
    size_t with_terms = 0;
    for (size_t k = 0; k < K; k++) with_terms += p.moff[k + 1] != p.moff[k];
    out3[0] = with_terms; out3[1] = p.perm.size(); out3[2] = p.large.size();
}
// n_before NULL: the plain aggregation
int emu_halfagg_inc_aggregate_batch(int32_t* results, unsigned char* out, const unsigned char* aggsigs_in, const uint64_t* n_before, const unsigned char* pks,
                                    int pk_format, const unsigned char* msgs32, const unsigned char* new_sigs64, const uint64_t* item_off, size_t K) {
    if (K == 0) return 1;
    if (!results || !out || pk_format < 0 || pk_format > 1 || !offsets_ok(item_off, K) || (n_before && !aggsigs_in)) return 0;
    if (item_off[K] && (!pks || !msgs32)) return 0;
    const size_t N = (size_t)item_off[K];
    std::vector<uint64_t> in_off(K + 1, 0), new_off(K + 1, 0);
    std::vector<u32> all(K);
    for (size_t k = 0; k < K; k++) {
        const uint64_t n = item_off[k + 1] - item_off[k], nb = n_before ? n_before[k] : 0;
        if (nb > n) return 0;
        in_off[k + 1] = in_off[k] + 32 * (nb + 1); new_off[k + 1] = new_off[k] + (n - nb); all[k] = (u32)k;
    }
    if (new_off[K] && !new_sigs64) return 0;
    for (size_t k = 0; k < K; k++) results[k] = 0;
    memset(out, 0, 32 * (N + K));
    const std::vector<u32> perm = hab_chain_order(item_off, all);
    std::vector<unsigned char> t32(32 * N + 1, 0xEE);
    std::vector<u32> states(8 * (hab_state_slot(N) + 1), 0xEEEEEEEEu), fail(K, 0);
    const hab_agg_view v{item_off, n_before ? in_off.data() : nullptr, new_off.data(), K, pks, pk_format, msgs32, aggsigs_in, new_sigs64, out, t32.data(), states.data(), fail.data()};
    for (size_t i = 0; i < N; i++) hab_gather_item(v, i);
    for (size_t lane = 0; lane < perm.size(); lane++) {
        const size_t k = perm[lane]; const uint64_t first = item_off[k];
        hab_chain_lane(states.data() + 8 * hab_state_slot(first), out + 32 * (first + k), pks + (pk_format ? 64 : 32) * first, pk_format, msgs32 + 32 * first,
                       (size_t)(item_off[k + 1] - first));
    }
    for (size_t i = 0; i < N; i++) hab_term_item(v, i);
    for (size_t k = 0; k < K; k++) results[k] = hab_sum_agg(v, k);
    return 1;
}
int emu_halfagg_aggregate_batch(int32_t* results, unsigned char* out, const unsigned char* pks, int pk_format, const unsigned char* msgs32, const unsigned char* sigs64,
                                const uint64_t* item_off, size_t K) {
    return emu_halfagg_inc_aggregate_batch(results, out, nullptr, nullptr, pks, pk_format, msgs32, sigs64, item_off, K);
}
}
