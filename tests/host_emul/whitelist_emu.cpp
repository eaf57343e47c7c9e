// tests/host_emul/whitelist_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/whitelist.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table and lane
// memory: that file is included as it is, so this library carries its own copy of both and is loaded next to libs2k_hostemu.so.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/whitelist.h"
#include <vector>

extern "C" {
// one pair: K = online + t (offline + sub) as x | y big-endian and the infinity flag; returns wl_key_lane's value
int emu_whitelist_key(unsigned char* xy64, int* inf, const unsigned char* online64, const unsigned char* offline64, const unsigned char* sub64) {
    u32 rec[WL_KEY_WORDS];
    const int ok = wl_key_lane(rec, online64, offline64, sub64, 1, gtab_host(), g_lm);
    gej K; gej_load28_h(K, rec);
    *inf = K.inf;
    for (int i = 0; i < 64; i++) xy64[i] = 0;
    if (!K.inf) { ge a; ge_set_gej(a, K); fe_to_b32(xy64, a.x); fe_to_b32(xy64 + 32, a.y); }
    return ok;
}
// one item, the arguments of secp256k1_whitelist_signature_parse + secp256k1_whitelist_verify: the two lane routines one after the
// other, with the planning rule of the batch entry points in between (an item that is not planned takes no key lanes)
int emu_whitelist_verify(const unsigned char* sig, size_t siglen, const unsigned char* online64, const unsigned char* offline64, size_t n_keys,
                         const unsigned char* sub64) {
    const size_t nk = wl_item_planned(n_keys, siglen) ? n_keys : 0;
    std::vector<u32> keys(WL_KEY_WORDS * nk + 1);
    for (size_t j = 0; j < nk; j++) wl_key_lane(keys.data() + WL_KEY_WORDS * j, online64 + 64 * j, offline64 + 64 * j, sub64, 1, gtab_host(), g_lm);
    u32 msg8[8];
    return wl_ring_lane(sig, siglen, keys.data(), online64, offline64, n_keys, sub64, msg8, 1, gtab_host(), g_lm);
}
}
