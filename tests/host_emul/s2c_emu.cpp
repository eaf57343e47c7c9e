// tests/host_emul/s2c_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/s2c.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits) and lane memory: that file is included as it is, so this library carries its own copy of both and is loaded next to
// libs2k_hostemu.so.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/s2c.h"

static const s2c_midstates& s2c_mid() {
    static s2c_midstates m; static int have = 0;
    if (!have) { s2c_tag_midstates(m); have = 1; }
    return m;
}

extern "C" {
// the arguments of secp256k1_ecdsa_s2c_verify_commit_batch / secp256k1_anti_exfil_host_verify_batch, one item; siglen is only read for DER
int emu_s2c_commit(const unsigned char* sig, size_t siglen, int sig_format, const unsigned char* data32, const unsigned char* opening, int opening_format) {
    return s2c_commit_lane(s2c_mid(), sig, siglen, sig_format, data32, opening, opening_format, 1, gtab_host());
}
int emu_s2c_host_verify(const unsigned char* sig, size_t siglen, int sig_format, const unsigned char* msghash32, const unsigned char* pk, int pk_format,
                        const unsigned char* host_data32, const unsigned char* opening, int opening_format) {
    return s2c_host_verify_lane(s2c_mid(), sig, siglen, sig_format, msghash32, pk, pk_format, host_data32, opening, opening_format, 1, gtab_host(), g_lm);
}
void emu_s2c_host_commit(unsigned char* out32, const unsigned char* rand32) { s2c_host_commit_lane(out32, s2c_mid(), rand32); }
// the tweak alone; returns whether the opening loaded
int emu_s2c_tweak(unsigned char* t32, const unsigned char* data32, const unsigned char* opening, int opening_format) {
    ge O; const int ok = s2c_opening_load(O, opening, opening_format);
    s2c_tweak(t32, s2c_mid(), O, data32);
    return ok;
}
// both midstates as 8 + 8 big-endian words: point, then data
void emu_s2c_midstates(unsigned char* out64) {
    for (int i = 0; i < 8; i++) { s2k_store_be32(out64 + 4 * i, s2c_mid().point[i]); s2k_store_be32(out64 + 32 + 4 * i, s2c_mid().data[i]); }
}
// s2c_x_matches on the point (x, y) scaled by z: (x z^2, y z^3, z); x | y and z big-endian, r big-endian and < n
int emu_s2c_x_matches(const unsigned char* xy64, const unsigned char* z32, const unsigned char* r32) {
    ge a; ge_from_b64(a, xy64);
    fe z, z2, z3; fe_from_b32(z, z32);
    gej R; R.inf = 0;
    fe_sqr(z2, z); fe_mul(z3, z2, z); fe_mul(R.x, a.x, z2); fe_mul(R.y, a.y, z3); R.z = z; fe_norm_weak(R.z);
    scalar r; sc_set_b32(r, r32, nullptr);
    return s2c_x_matches(R, r);
}
}
