// tests/host_emul/musig_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/musig.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits): that file is included as it is, so this library carries its own copy of the table and is loaded next to libs2k_hostemu.so.
// With -DMUSIG_EMU_MAIN the file is a stand-alone program (for -fsanitize=address,undefined builds: nothing loaded into an interpreter
// is sanitised) that reads items as hex lines on standard input and prints one result per line.
static unsigned long long g_joint_done = 0;
#define S2K_ON_JOINT_DONE() (g_joint_done++)
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/musig.h"

extern "C" {
// one item of secp256k1_musig_partial_sig_verify_batch with its own cache and session
int emu_musig_verify(const unsigned char* sig, int sig_format, const unsigned char* pubnonce, int nonce_format, const unsigned char* pubkey, int pk_format,
                     const unsigned char* cache197, const unsigned char* session133) {
    musig_midstates mid; musig_tag_midstates(mid);
    u32 park[S2K_MUSIG_PARK_WORDS]; memset(park, 0xA5, sizeof(park));
    return musig_verify_lane(mid, sig, sig_format, pubnonce, nonce_format, pubkey, pk_format, cache197, session133, 1, nullptr, 0, 1, gtab_host(), g_lm, park, 0, 1);
}
// ... through session_of: item 0 of the arrays, pair session_index of n_sessions
int emu_musig_verify_indexed(const unsigned char* sig, int sig_format, const unsigned char* pubnonce, int nonce_format, const unsigned char* pubkey, int pk_format,
                             const unsigned char* caches, const unsigned char* sessions, size_t n_sessions, unsigned session_index) {
    musig_midstates mid; musig_tag_midstates(mid);
    u32 park[S2K_MUSIG_PARK_WORDS]; memset(park, 0xA5, sizeof(park));
    const u32 of[1] = {session_index};
    return musig_verify_lane(mid, sig, sig_format, pubnonce, nonce_format, pubkey, pk_format, caches, sessions, n_sessions, of, 0, 1, gtab_host(), g_lm, park, 0, 1);
}
unsigned long long emu_musig_joint_count(void) { return g_joint_done; }
// one item of secp256k1_musig_nonce_process_batch; adaptor64 NULL: the adaptor-free kernel
int emu_musig_process(unsigned char* session_out133, const unsigned char* aggnonce, int nonce_format, const unsigned char* msg32, const unsigned char* cache197,
                      const unsigned char* adaptor64) {
    musig_midstates mid; musig_tag_midstates(mid);
    u32 park[S2K_MUSIG_PARK_R1_WORDS]; memset(park, 0xA5, sizeof(park));
    if (adaptor64) return musig_process_lane<1>(mid, session_out133, aggnonce, nonce_format, msg32, cache197, adaptor64, 0, 1, gtab_host(), g_lm, park, 0, 1);
    return musig_process_lane<0>(mid, session_out133, aggnonce, nonce_format, msg32, cache197, nullptr, 0, 1, gtab_host(), g_lm, park, 0, 1);
}
// the three midstates the engine computes: 3 x eight big-endian words (KeyAgg coefficient | MuSig/noncecoef | BIP0340/challenge)
void emu_musig_midstates(unsigned char* out96) {
    musig_midstates mid; musig_tag_midstates(mid);
    for (int i = 0; i < 8; i++) { s2k_store_be32(out96 + 4 * i, mid.coef[i]); s2k_store_be32(out96 + 32 + 4 * i, mid.noncecoef[i]); s2k_store_be32(out96 + 64 + 4 * i, mid.challenge[i]); }
}
}

#ifdef MUSIG_EMU_MAIN
#include <stdio.h>
#include <string>
#include <iostream>
static int unhex(std::vector<unsigned char>& out, const std::string& s) {
    if (s.size() % 2) return 0;
    out.clear();
    for (size_t i = 0; i < s.size(); i += 2) { unsigned v; if (sscanf(s.c_str() + i, "%2x", &v) != 1) return 0; out.push_back((unsigned char)v); }
    return 1;
}
// each line, hex fields blank separated:   v sig_format nonce_format pk_format sig pubnonce pubkey cache session   -> "verdict"
//                                          p nonce_format aggnonce msg32 cache adaptor|-                          -> "verdict session-hex"
int main() {
    std::string kind;
    while (std::cin >> kind) {
        if (kind == "v") {
            std::string f0, f1, f2, a, b, c, d, e;
            if (!(std::cin >> f0 >> f1 >> f2 >> a >> b >> c >> d >> e)) { printf("bad line\n"); return 2; }
            const int sf = atoi(f0.c_str()), nf = atoi(f1.c_str()), pf = atoi(f2.c_str());
            std::vector<unsigned char> sig, nonce, pk, cache, sess;
            if (sf < 0 || sf > 1 || nf < 0 || nf > 1 || pf < 0 || pf > 2 || !unhex(sig, a) || !unhex(nonce, b) || !unhex(pk, c) || !unhex(cache, d) || !unhex(sess, e) ||
                sig.size() != musig_sig_bytes(sf) || nonce.size() != musig_nonce_bytes(nf) || pk.size() != ecdsa_pk_bytes(pf) || cache.size() != 197 || sess.size() != 133) { printf("bad line\n"); return 2; }
            printf("%d\n", emu_musig_verify(sig.data(), sf, nonce.data(), nf, pk.data(), pf, cache.data(), sess.data()));
        } else if (kind == "p") {
            std::string f, a, b, c, d;
            if (!(std::cin >> f >> a >> b >> c >> d)) { printf("bad line\n"); return 2; }
            const int nf = atoi(f.c_str());
            std::vector<unsigned char> nonce, msg, cache, ad;
            if (nf < 0 || nf > 1 || !unhex(nonce, a) || !unhex(msg, b) || !unhex(cache, c) || (d != "-" && !unhex(ad, d)) || nonce.size() != musig_nonce_bytes(nf) ||
                msg.size() != 32 || cache.size() != 197 || (d != "-" && ad.size() != 64)) { printf("bad line\n"); return 2; }
            unsigned char out[133];
            const int r = emu_musig_process(out, nonce.data(), nf, msg.data(), cache.data(), d == "-" ? nullptr : ad.data());
            printf("%d ", r);
            for (int i = 0; i < 133; i++) printf("%02x", out[i]);
            printf("\n");
        } else { printf("bad line\n"); return 2; }
    }
    return 0;
}
#endif
