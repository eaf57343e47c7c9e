// tests/host_emul/tweak_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/tweak.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits): that file is included as it is, so this library carries its own copy of the table and is loaded next to libs2k_hostemu.so.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/tweak.h"

extern "C" {
// the arguments of secp256k1_xonly_pubkey_tweak_add_check_batch, one item; parity is the item's byte
int emu_tweak_check(const unsigned char* tweaked32, unsigned parity, const unsigned char* key, int key_format, const unsigned char* tweak32) {
    return tweak_check_lane(tweaked32, parity, key, key_format, tweak32, 1, gtab_host());
}
int emu_tweak_add(unsigned char* pubkey_out64, const unsigned char* key, int key_format, const unsigned char* tweak32) {
    return tweak_add_lane(pubkey_out64, key, key_format, tweak32, 1, gtab_host());
}
// t * G through the fixed-base routine alone (t big-endian, reduced mod n): x | y big-endian; returns the infinity flag
int emu_tweak_gmul(unsigned char* xy64, const unsigned char* t32) {
    scalar t; sc_set_b32(t, t32, nullptr);
    gej T; tweak_gmul_fixed(T, gtab_host(), t.d);
    return gej_to_b64(xy64, T);
}
unsigned emu_tweak_gtab_bits(void) { return gtab_host()[0]; }
}
