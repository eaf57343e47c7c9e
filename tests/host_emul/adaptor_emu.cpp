// tests/host_emul/adaptor_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/adaptor.h and ecmult_lane2 (ecmult.h) compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built
// generator table (12-bit digits): that file is included as it is, so this library carries its own copy of the table and is loaded next
// to libs2k_hostemu.so.  With -DADAPTOR_EMU_MAIN the file is a stand-alone program (for -fsanitize=address,undefined builds: nothing
// loaded into an interpreter is sanitised) that reads items as hex lines on standard input and prints one verdict per line.
static unsigned long long g_joint_done = 0;
#define S2K_ON_JOINT_DONE() (g_joint_done++)
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/adaptor.h"

extern "C" {
// the arguments of secp256k1_ecdsa_adaptor_verify_batch, one item
int emu_adaptor_verify(const unsigned char* sig162, const unsigned char* pubkey, const unsigned char* msg32, const unsigned char* enckey, int pk_format) {
    adaptor_midstate mid; adaptor_tag_midstate(mid);
    u32 park[S2K_ADAPTOR_PARK_WORDS]; memset(park, 0xA5, sizeof(park));
    return adaptor_verify_lane(mid, sig162, pubkey, msg32, enckey, 0, pk_format, 1, gtab_host(), g_lm, park, 0, 1);
}
unsigned long long emu_adaptor_joint_count(void) { return g_joint_done; }
// na*A + nb*B as the kernels take it: the joint form, then the two-call form when it declines; *took_joint = 1 when the joint form
// produced the result.  x | y big-endian; returns the infinity flag
int emu_ecmult2(unsigned char* r64, int* took_joint, const unsigned char* a64, int ainf, const unsigned char* na32, const unsigned char* b64, int binf,
                const unsigned char* nb32) {
    ge a, b; gej A, B, R; scalar na, nb;
    ge_from_b64(a, a64); ge_from_b64(b, b64);
    fe_norm_weak(a.x); fe_norm_weak(a.y); fe_norm_weak(b.x); fe_norm_weak(b.y);
    gej_set_ge(A, a); gej_set_ge(B, b); A.inf = ainf != 0; B.inf = binf != 0;
    sc_set_b32(na, na32, nullptr); sc_set_b32(nb, nb32, nullptr);
    u32 park[S2K_PARK_GEJ_WORDS];
    const int done = ecmult_lane2(R, A, na, B, nb, g_lm);
    if (!done) ecmult_lane2_calls(R, [&](int k, gej& Pj, scalar& n) { Pj = k ? B : A; n = k ? nb : na; }, gtab_host(), g_lm, park, 1);
    *took_joint = done;
    return gej_to_b64(r64, R);
}
// the midstate the engine computes: eight big-endian words
void emu_adaptor_midstate(unsigned char* out32) {
    adaptor_midstate mid; adaptor_tag_midstate(mid);
    for (int i = 0; i < 8; i++) s2k_store_be32(out32 + 4 * i, mid.s[i]);
}
// the challenge over five serialised points (165 bytes), reduced mod n, 32 big-endian bytes
void emu_adaptor_challenge(unsigned char* e32, const unsigned char* points165) {
    adaptor_midstate mid; adaptor_tag_midstate(mid);
    u32 xw[5][8], pre[5];
    for (int k = 0; k < 5; k++) adaptor_words_b33(xw[k], pre[k], points165 + 33 * k);
    scalar e; adaptor_challenge(e, mid, xw, pre);
    sc_get_b32(e32, e);
}
}

#ifdef ADAPTOR_EMU_MAIN
#include <stdio.h>
#include <string>
#include <iostream>
static int unhex(std::vector<unsigned char>& out, const std::string& s) {
    if (s.size() % 2) return 0;
    out.clear();
    for (size_t i = 0; i < s.size(); i += 2) { unsigned v; if (sscanf(s.c_str() + i, "%2x", &v) != 1) return 0; out.push_back((unsigned char)v); }
    return 1;
}
// each line: pk_format sig162 pubkey msg32 enckey (hex, blank separated) -> "verdict"
int main() {
    std::string f, a, b, c, d;
    while (std::cin >> f >> a >> b >> c >> d) {
        std::vector<unsigned char> sig, pk, msg, ek;
        const int fmt = atoi(f.c_str());
        const size_t kb = fmt == 0 ? 33 : fmt == 1 ? 64 : 65;
        if (fmt < 0 || fmt > 2 || !unhex(sig, a) || !unhex(pk, b) || !unhex(msg, c) || !unhex(ek, d) || sig.size() != 162 || pk.size() != kb || msg.size() != 32 || ek.size() != kb) { printf("bad line\n"); return 2; }
        printf("%d\n", emu_adaptor_verify(sig.data(), pk.data(), msg.data(), ek.data(), fmt));
    }
    return 0;
}
#endif
