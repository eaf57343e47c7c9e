// tests/host_emul/ecdsa_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/ecdsa.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table and lane
// memory: that file is included as it is, so this library carries its own copy of both and is loaded next to libs2k_hostemu.so.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/ecdsa.h"

extern "C" {
// sig_format / pk_format as secp256k1_ecdsa_verify_batch; siglen is only read for DER
int emu_ecdsa_verify(const unsigned char* sig, size_t siglen, int sig_format, const unsigned char* msghash32, const unsigned char* pk, int pk_format) {
    return ecdsa_verify_lane(sig, siglen, sig_format, msghash32, pk, pk_format, 1, gtab_host(), g_lm);
}
int emu_ecdsa_recover(unsigned char* pubkey_out64, const unsigned char* sig64, unsigned recid, const unsigned char* msghash32) {
    return ecdsa_recover_lane(pubkey_out64, sig64, recid, msghash32, 1, gtab_host(), g_lm);
}
// the parsers alone: r and s as 32 big-endian bytes each / the point as x | y big-endian
int emu_ecdsa_sig_load(unsigned char* rs64, const unsigned char* sig, size_t siglen, int sig_format) {
    scalar r, s; const int ok = ecdsa_sig_load(r, s, sig, siglen, sig_format);
    sc_get_b32(rs64, r); sc_get_b32(rs64 + 32, s);
    return ok;
}
int emu_ecdsa_pubkey_load(unsigned char* xy64, const unsigned char* pk, int pk_format) {
    ge P; const int ok = ecdsa_pubkey_load(P, pk, pk_format);
    fe_to_b32(xy64, P.x); fe_to_b32(xy64 + 32, P.y);
    return ok;
}
}
