// tests/host_emul/musig_agg_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/musig_agg.h compiled for the host (S2K_VERIFY on), on top of hostemu.cpp's host-built generator table (12-bit
// digits): that file is included as it is, so this library carries its own copy of the table and is loaded next to libs2k_hostemu.so.
// The batch functions drive the stages the way engine_musig_agg.hip plans them: the same plan (musig_agg_plan_sum), the same per-item
// functions, one "lane" after the other, scratch arrays of exactly the planned sizes.
// With -DMUSIG_AGG_EMU_MAIN the file is a stand-alone program (for -fsanitize=address,undefined builds: nothing loaded into an
// interpreter is sanitised) that reads calls as hex lines on standard input and prints one result per line.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/musig_agg.h"

// the passes over the partials in `a`; returns the buffer that holds the nseg sums
static std::vector<u32>& emu_sum(const musig_agg_sum_plan& p, std::vector<u32>& a, std::vector<u32>& b, unsigned fanin) {
    std::vector<u32>* in = &a; std::vector<u32>* out = &b;
    for (size_t q = 0; q < p.passes; q++) {
        const uint64_t* in_off = p.offs.data() + q * (p.nseg + 1); const uint64_t* out_off = in_off + p.nseg + 1;
        const size_t total = (size_t)out_off[p.nseg];
        for (size_t j = 0; j < total; j++) musig_agg_sum_item(out->data(), in->data(), in_off, out_off, p.nseg, fanin, j);
        std::swap(in, out);
    }
    return *in;
}

extern "C" {
int emu_musig_pubkey_agg(int* results, unsigned char* caches197, unsigned char* agg_pks64, const unsigned char* pubkeys, int pk_format, const uint64_t* set_off,
                         size_t n_sets, unsigned fanin) {
    if (fanin < 2 || fanin > MUSIG_AGG_FANIN_MAX || pk_format < 0 || pk_format > 2) return 0;
    const musig_agg_sum_plan p = musig_agg_plan_sum(set_off, n_sets, fanin);
    const size_t n_keys = (size_t)set_off[n_sets];
    std::vector<u32> a((size_t)MUSIG_AGG_GEJ_WORDS * p.cap), b((size_t)MUSIG_AGG_GEJ_WORDS * p.cap), second(n_sets);
    std::vector<int32_t> key_ok(n_keys);
    std::vector<unsigned char> pks_hash(32 * n_sets);
    musig_agg_mids mid; musig_agg_midstates(mid);
    for (size_t k = 0; k < n_sets; k++) musig_agg_list_lane(pks_hash.data() + 32 * k, second.data() + k, mid.list, pubkeys, pk_format, set_off[k], set_off[k + 1] - set_off[k]);
    for (size_t i = 0; i < n_keys; i++) {
        const size_t k = (size_t)musig_agg_segment(set_off, n_sets, i);
        key_ok[i] = musig_agg_term_lane(a.data() + (size_t)MUSIG_AGG_GEJ_WORDS * i, mid.coef, pubkeys, pk_format, i, set_off[k], second[k], pks_hash.data() + 32 * k, 1,
                                        gtab_host(), g_lm);
    }
    const std::vector<u32>& sums = emu_sum(p, a, b, fanin);
    for (size_t k = 0; k < n_sets; k++)
        results[k] = musig_agg_finish_lane(caches197 + 197 * k, agg_pks64 ? agg_pks64 + 64 * k : nullptr, sums.data() + (size_t)MUSIG_AGG_GEJ_WORDS * k, key_ok.data(), set_off[k],
                                           set_off[k + 1] - set_off[k], pks_hash.data() + 32 * k, second[k], pubkeys, pk_format, 1);
    return 1;
}
// caches_out197 may be caches_in197
int emu_musig_pubkey_tweak_add(int* results, unsigned char* caches_out197, unsigned char* pubkeys_out64, const unsigned char* caches_in197, const unsigned char* tweaks32,
                               const unsigned char* xonly, size_t n) {
    for (size_t i = 0; i < n; i++)
        results[i] = musig_agg_tweak_lane(caches_out197 + 197 * i, pubkeys_out64 ? pubkeys_out64 + 64 * i : nullptr, caches_in197 + 197 * i, tweaks32 + 32 * i,
                                          xonly ? (unsigned)xonly[i] : 0u, 1, gtab_host());
    return 1;
}
int emu_musig_nonce_agg(int* results, unsigned char* aggnonces_out, int out_format, const unsigned char* pubnonces, int nonce_format, const uint64_t* nonce_off,
                        size_t n_sessions, unsigned fanin) {
    if (fanin < 2 || fanin > MUSIG_AGG_FANIN_MAX || out_format < 0 || out_format > 1 || nonce_format < 0 || nonce_format > 1) return 0;
    const musig_agg_sum_plan p = musig_agg_plan_nonces(nonce_off, n_sessions, fanin);
    const size_t n = (size_t)nonce_off[n_sessions];
    std::vector<u32> a((size_t)MUSIG_AGG_GEJ_WORDS * p.cap), b((size_t)MUSIG_AGG_GEJ_WORDS * p.cap);
    std::vector<int32_t> nonce_ok(n);
    for (size_t i = 0; i < n; i++)
        nonce_ok[i] = musig_agg_nonce_load_lane(a.data() + (size_t)MUSIG_AGG_GEJ_WORDS * i, a.data() + (size_t)MUSIG_AGG_GEJ_WORDS * (n + i),
                                                pubnonces + musig_nonce_bytes(nonce_format) * i, nonce_format, 1);
    const std::vector<u32>& sums = emu_sum(p, a, b, fanin);
    for (size_t k = 0; k < n_sessions; k++)
        results[k] = musig_agg_nonce_finish_lane(aggnonces_out + musig_nonce_bytes(out_format) * k, out_format, sums.data() + (size_t)MUSIG_AGG_GEJ_WORDS * k,
                                                 sums.data() + (size_t)MUSIG_AGG_GEJ_WORDS * (n_sessions + k), nonce_ok.data(), nonce_off[k], nonce_off[k + 1] - nonce_off[k], 1);
    return 1;
}
int emu_musig_partial_sig_agg(int* results, unsigned char* sigs64_out, const unsigned char* sessions133, const unsigned char* partial_sigs, int sig_format,
                              const uint64_t* sig_off, size_t n_sessions) {
    if (sig_format < 0 || sig_format > 1) return 0;
    for (size_t k = 0; k < n_sessions; k++)
        results[k] = musig_agg_sig_lane(sigs64_out + 64 * k, sessions133 + 133 * k, partial_sigs, sig_format, sig_off[k], sig_off[k + 1] - sig_off[k], 1);
    return 1;
}
// the "KeyAgg list" midstate the engine computes: eight big-endian words
void emu_musig_agg_list_midstate(unsigned char* out32) {
    musig_agg_mids mid; musig_agg_midstates(mid);
    for (int i = 0; i < 8; i++) s2k_store_be32(out32 + 4 * i, mid.list[i]);
}
// the plan of a sum: passes, and the most partials any array holds
size_t emu_musig_agg_plan(const uint64_t* off, size_t nseg, unsigned fanin, size_t* cap) {
    const musig_agg_sum_plan p = musig_agg_plan_sum(off, nseg, fanin);
    if (cap) *cap = p.cap;
    return p.passes;
}
}

#ifdef MUSIG_AGG_EMU_MAIN
#include <stdio.h>
#include <string>
#include <iostream>
static int unhex(std::vector<unsigned char>& out, const std::string& s) {
    out.clear();
    if (s == "-") return 1;
    if (s.size() % 2) return 0;
    for (size_t i = 0; i < s.size(); i += 2) { unsigned v; if (sscanf(s.c_str() + i, "%2x", &v) != 1) return 0; out.push_back((unsigned char)v); }
    return 1;
}
static void put(const unsigned char* p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", p[i]); }
static int fail() { printf("bad line\n"); return 2; }
// each line is ONE item (one set / cache / session), fields blank separated, "-" an empty byte string:
//   k pk_format fanin keys                  -> "verdict cache agg_pk"
//   t xonly_byte cache tweak32              -> "verdict cache_out pubkey_out"        (in place)
//   n nonce_format out_format fanin nonces  -> "verdict aggnonce"
//   s sig_format session sigs               -> "verdict sig64"
// Buffers are heap vectors of exactly the bytes given, so that a read past an item's end is the sanitizer's to find.
int main() {
    std::string kind;
    while (std::cin >> kind) {
        if (kind == "k") {
            std::string f, fi, a; if (!(std::cin >> f >> fi >> a)) return fail();
            const int pf = atoi(f.c_str()); const unsigned fan = (unsigned)atoi(fi.c_str());
            std::vector<unsigned char> keys; if (pf < 0 || pf > 2 || !unhex(keys, a) || keys.size() % ecdsa_pk_bytes(pf)) return fail();
            const uint64_t off[2] = {0, keys.size() / ecdsa_pk_bytes(pf)};
            std::vector<unsigned char> cache(197), agg(64); int r = 0;
            if (!emu_musig_pubkey_agg(&r, cache.data(), agg.data(), keys.data(), pf, off, 1, fan)) return fail();
            printf("%d ", r); put(cache.data(), 197); printf(" "); put(agg.data(), 64); printf("\n");
        } else if (kind == "t") {
            std::string x, a, b; if (!(std::cin >> x >> a >> b)) return fail();
            std::vector<unsigned char> cache, tw, xo(1, (unsigned char)atoi(x.c_str())), pk(64); int r = 0;
            if (!unhex(cache, a) || !unhex(tw, b) || cache.size() != 197 || tw.size() != 32) return fail();
            emu_musig_pubkey_tweak_add(&r, cache.data(), pk.data(), cache.data(), tw.data(), xo.data(), 1);
            printf("%d ", r); put(cache.data(), 197); printf(" "); put(pk.data(), 64); printf("\n");
        } else if (kind == "n") {
            std::string f, o, fi, a; if (!(std::cin >> f >> o >> fi >> a)) return fail();
            const int nf = atoi(f.c_str()), of = atoi(o.c_str()); const unsigned fan = (unsigned)atoi(fi.c_str());
            std::vector<unsigned char> nonces; if (nf < 0 || nf > 1 || of < 0 || of > 1 || !unhex(nonces, a) || nonces.size() % musig_nonce_bytes(nf)) return fail();
            const uint64_t off[2] = {0, nonces.size() / musig_nonce_bytes(nf)};
            std::vector<unsigned char> out(musig_nonce_bytes(of)); int r = 0;
            if (!emu_musig_nonce_agg(&r, out.data(), of, nonces.data(), nf, off, 1, fan)) return fail();
            printf("%d ", r); put(out.data(), out.size()); printf("\n");
        } else if (kind == "s") {
            std::string f, a, b; if (!(std::cin >> f >> a >> b)) return fail();
            const int sf = atoi(f.c_str());
            std::vector<unsigned char> sess, sigs; if (sf < 0 || sf > 1 || !unhex(sess, a) || !unhex(sigs, b) || sess.size() != 133 || sigs.size() % musig_sig_bytes(sf)) return fail();
            const uint64_t off[2] = {0, sigs.size() / musig_sig_bytes(sf)};
            std::vector<unsigned char> out(64); int r = 0;
            if (!emu_musig_partial_sig_agg(&r, out.data(), sess.data(), sigs.data(), sf, off, 1)) return fail();
            printf("%d ", r); put(out.data(), 64); printf("\n");
        } else return fail();
    }
    return 0;
}
#endif
