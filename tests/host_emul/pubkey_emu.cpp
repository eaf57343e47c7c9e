// tests/host_emul/pubkey_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/pubkey.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits): that file is included as it is, so this library carries its own copy of the table and is loaded next to libs2k_hostemu.so.
// The combine function drives the stages the way engine_pubkey.hip plans them: the same plan (musig_agg_plan_sum), pass 0 through
// pubkey_fold_item (or, for the formats with a square root, pubkey_partial_lane and every pass), the passes through musig_agg_sum_item,
// one "lane" after the other, scratch arrays of exactly the planned sizes.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/pubkey.h"

extern "C" {
// one item of secp256k1_ec_pubkey_convert_batch / _negate_batch; parity_out may be NULL
int emu_pubkey_convert(unsigned char* out, int out_format, unsigned char* parity_out, const unsigned char* in, int in_format, int negate) {
    if (!pubkey_out_format_ok(out_format) || !pubkey_in_format_ok(in_format)) return -1;
    return pubkey_convert_lane(out, out_format, parity_out, in, in_format, negate, 1);
}
// one item of secp256k1_ec_pubkey_tweak_mul_batch
int emu_pubkey_tweak_mul(unsigned char* out, int out_format, unsigned char* parity_out, const unsigned char* key, int key_format, const unsigned char* tweak32) {
    if (!pubkey_out_format_ok(out_format) || !pubkey_in_format_ok(key_format)) return -1;
    return pubkey_tweak_mul_lane(out, out_format, parity_out, key, key_format, tweak32, 1, gtab_host(), g_lm);
}
// secp256k1_ec_pubkey_combine_batch; passes_out (may be NULL) receives the plan's number of passes
int emu_pubkey_combine(int* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* keys, int key_format, const uint64_t* key_off,
                       size_t n_sets, unsigned fanin, size_t* passes_out) {
    if (fanin < 2 || fanin > PUBKEY_FOLD_FANIN_MAX || !pubkey_out_format_ok(out_format) || !pubkey_in_format_ok(key_format)) return 0;
    const musig_agg_sum_plan p = musig_agg_plan_sum(key_off, n_sets, fanin);
    if (passes_out) *passes_out = p.passes;
    // formats whose load is a square root take the load-then-fold chain (one key per "lane" to a partial, then every pass); the others
    // the fused pass 0
    const int fused = key_format != S2K_PK_XONLY && key_format != S2K_PK_COMPRESSED;
    size_t cap = fused ? 0 : p.cap;
    for (size_t q = 1; fused && q <= p.passes; q++) cap = std::max(cap, (size_t)p.offs[q * (n_sets + 1) + n_sets]);
    const uint64_t* flag_off = p.offs.data() + (fused ? n_sets + 1 : 0);
    const size_t n_flags = (size_t)flag_off[n_sets];
    std::vector<u32> a((size_t)MUSIG_AGG_GEJ_WORDS * cap), b((size_t)MUSIG_AGG_GEJ_WORDS * cap);
    std::vector<int32_t> flag(n_flags);
    std::vector<u32>* in = &a; std::vector<u32>* outv = &b;
    if (fused) {
        for (size_t j = 0; j < n_flags; j++) flag[j] = pubkey_fold_item(b.data(), keys, key_format, p.offs.data(), flag_off, n_sets, fanin, j);
        std::swap(in, outv);
    } else {
        for (size_t i = 0; i < n_flags; i++) flag[i] = pubkey_partial_lane(a.data() + (size_t)MUSIG_AGG_GEJ_WORDS * i, keys + pubkey_bytes(key_format) * i, key_format);
    }
    for (size_t q = fused ? 1 : 0; q < p.passes; q++) {
        const uint64_t* qi = p.offs.data() + q * (n_sets + 1); const uint64_t* qo = qi + n_sets + 1;
        for (size_t j = 0; j < (size_t)qo[n_sets]; j++) musig_agg_sum_item(outv->data(), in->data(), qi, qo, n_sets, fanin, j);
        std::swap(in, outv);
    }
    const size_t ob = pubkey_bytes(out_format);
    for (size_t k = 0; k < n_sets; k++)
        results[k] = pubkey_combine_finish_lane(out + ob * k, out_format, parities_out ? parities_out + k : nullptr, in->data() + (size_t)MUSIG_AGG_GEJ_WORDS * k, flag.data(),
                                                flag_off[k], flag_off[k + 1] - flag_off[k], key_off[k + 1] - key_off[k], 1);
    return 1;
}
size_t emu_pubkey_bytes(int format) { return pubkey_bytes(format); }
unsigned emu_pubkey_fanin_default(void) { return PUBKEY_FOLD_FANIN_DEFAULT; }
}
