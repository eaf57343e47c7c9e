// tests/host_emul/generator_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/generator.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits): that file is included as it is, so this library carries its own copy of the table and is loaded next to libs2k_hostemu.so.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/generator.h"

extern "C" {
// the bare map: t32 big-endian (>= p: returns -1) -> x | y big-endian, normalised; returns the branch taken (0, 1, 2 for x1, x2, x3).
// The inversion is the plain fe_inv, whose value at 0 is 0, as in the reference.
int emu_gen_map(unsigned char* xy64, const unsigned char* t32) {
    fe t, j, ji; ge p; int branch = -1;
    if (!fe_set_b32_limit(t, t32)) return -1;
    gen_map_j(j, t); fe_norm_weak(j);
    fe_inv(ji, j);
    gen_map_point(p, t, ji, &branch);
    fe_normalize(p.x); fe_normalize(p.y);
    fe_get_b32(xy64, p.x); fe_get_b32(xy64 + 32, p.y);
    return branch;
}
// generate from the two field elements the hashes would give (t >= p: returns -1); blind32 may be NULL
int emu_gen_from_t(unsigned char* gen_out64, const unsigned char* t1_32, const unsigned char* t2_32, const unsigned char* blind32) {
    fe t1, t2;
    if (!fe_set_b32_limit(t1, t1_32) || !fe_set_b32_limit(t2, t2_32)) return -1;
    return generator_from_t_lane(gen_out64, t1, t2, blind32, 1, 1, gtab_host());
}
// the per-item routines behind the four entry points
int emu_gen_generate(unsigned char* gen_out64, const unsigned char* key32, const unsigned char* blind32) {
    return generator_generate_lane(gen_out64, key32, blind32, 1, gtab_host());
}
int emu_gen_parse(unsigned char* gen_out64, const unsigned char* in33) { return generator_parse_lane(gen_out64, in33, 1); }
void emu_gen_serialize(unsigned char* out33, const unsigned char* gen64) { generator_serialize_lane(out33, gen64, 1); }
int emu_pedersen_commit(unsigned char* commit_out33, const unsigned char* blind32, unsigned long long value, const unsigned char* gen64) {
    u32 dig[S2K_DIG_WORDS]; const lane_mem lm{g_ptab, dig};
    return pedersen_commit_lane(commit_out33, blind32, (u64)value, gen64, 1, gtab_host(), lm);
}
}
