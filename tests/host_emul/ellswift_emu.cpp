// tests/host_emul/ellswift_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/ellswift.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp: that file is included as it is, so
// this library carries its own copy of it and is loaded next to libs2k_hostemu.so.  On the host fe_inv_lanes inverts per lane.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/ellswift.h"

static const ellswift_midstate& ellswift_mid() {
    static ellswift_midstate m; static int have = 0;
    if (!have) { ellswift_tag_midstate(m); have = 1; }
    return m;
}

extern "C" {
// secp256k1_ellswift_decode_batch, one item: out has ellswift_out_bytes(out_format) bytes
void emu_ellswift_decode(unsigned char* out, int out_format, const unsigned char* ell64) { ellswift_decode_lane(out, out_format, ell64, 1); }
// which of x3, x2, x1 the fraction routine takes (3, 2, 1), with two roots (x1 untested) or three
int emu_ellswift_which(const unsigned char* ell64, int roots) {
    fe u, t, xn, xd, root;
    fe_set_b32_mod(u, ell64); fe_set_b32_mod(t, ell64 + 32); fe_normalize(t);
    return roots == 2 ? ellswift_xswiftec_frac(xn, xd, u, t) : ellswift_frac_root(xn, xd, root, u, t, roots);
}
// the partial inverse: x, u big-endian; returns the flag and t (normalised, big-endian)
int emu_ellswift_inv(unsigned char* t32, const unsigned char* x32, const unsigned char* u32_, int c) {
    fe x, u, t;
    fe_set_b32_mod(x, x32); fe_set_b32_mod(u, u32_);
    const int ok = ellswift_xswiftec_inv(t, x, u, c);
    fe_normalize(t); fe_get_b32(t32, t);
    return ok;
}
// secp256k1_ellswift_encode_batch, one item
int emu_ellswift_encode(unsigned char* ell64, int* capped, const unsigned char* key, int key_format, const unsigned char* rnd32, unsigned max_attempts) {
    return ellswift_encode_lane(ell64, capped, ellswift_mid(), key, key_format, rnd32, 1, max_attempts);
}
// out[0..3] = pool counter, draw counter, byte and shift of the branch value of `attempt`
void emu_ellswift_schedule(unsigned* out, unsigned attempt) {
    out[0] = ellswift_pool_counter(attempt); out[1] = ellswift_draw_counter(attempt);
    ellswift_branch_index(out[2], out[3], attempt);
}
int emu_ellswift_branch_value(const unsigned char* pool32, unsigned attempt) {
    u32 w[8];
    for (int j = 0; j < 8; j++) w[j] = s2k_load_be32(pool32 + 4 * j);
    return ellswift_branch_value(w, attempt);
}
// the tag midstate as 8 big-endian words
void emu_ellswift_midstate(unsigned char* out32) { for (int i = 0; i < 8; i++) s2k_store_be32(out32 + 4 * i, ellswift_mid().s[i]); }
}
