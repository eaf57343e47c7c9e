// tests/host_emul/hash_batch_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// secp256k1_zkp_amd/csrc/hash_batch.h compiled for the host, on top of hostemu.cpp (included as it is, for schnorr_verify_lane and the
// host-built generator table): the per-lane routines behind s2k_sha256_batch, secp256k1_tagged_sha256_batch and
// secp256k1_schnorrsig_verify_batch_var, one "lane" after the other, with the item rule of the kernels (hash_item_span).  The tag's
// midstate is made with the byte-at-a-time context of sha256.h, so the word-reading routine is not its own witness there.
#include "hostemu.cpp"
#include "../../secp256k1_zkp_amd/csrc/hash_batch.h"

static hash_state emu_tag_midstate(const unsigned char* tag, size_t taglen) {
    sha256_stream h; sha256_stream_init(h);
    sha256_stream_write(h, tag, taglen);
    unsigned char th[32]; sha256_stream_finalize(h, th);
    sha256_stream g; sha256_stream_init(g);
    sha256_stream_write(g, th, 32); sha256_stream_write(g, th, 32);       // exactly one block: compressed
    hash_state m;
    for (int i = 0; i < 8; i++) m.s[i] = g.s[i];
    return m;
}

extern "C" {
// mode 0: SHA256, 1: SHA256 of SHA256, 2: tagged.  msg_off NULL: n items of msglen bytes; else item i is msgs[msg_off[i] .. msg_off[i+1])
int emu_hash_batch(unsigned char* out32, int mode, const unsigned char* tag, size_t taglen, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, size_t n) {
    if (mode < 0 || mode > 2) return 0;
    hash_state start;
    if (mode == 2) start = emu_tag_midstate(tag, taglen); else sha256_init(start.s);
    for (size_t i = 0; i < n; i++) {
        if (mode == 0) hash_batch_item<0, 0>(out32, start, msgs, (const u64*)msg_off, msglen, i);
        else if (mode == 1) hash_batch_item<0, 1>(out32, start, msgs, (const u64*)msg_off, msglen, i);
        else hash_batch_item<64, 0>(out32, start, msgs, (const u64*)msg_off, msglen, i);
    }
    return 1;
}
// one item whose message is its own pointer (hash_batch_bounds: every message in an allocation of exactly its length)
void emu_hash_one(unsigned char* out32, int mode, const unsigned char* tag, size_t taglen, const unsigned char* msg, size_t len) {
    hash_state start;
    if (mode == 2) start = emu_tag_midstate(tag, taglen); else sha256_init(start.s);
    if (mode == 0) hash_lane<0, 0>(out32, start, msg, len);
    else if (mode == 1) hash_lane<0, 1>(out32, start, msg, len);
    else hash_lane<64, 0>(out32, start, msg, len);
}
// secp256k1_schnorrsig_verify_batch_var, as k_schnorr_verify_var runs a lane
int emu_schnorr_verify_var(int* results, const unsigned char* sigs, const unsigned char* msgs, const uint64_t* msg_off, const unsigned char* pks, int pk_format, size_t n) {
    schnorr_midstate mid; schnorr_tag_midstate(mid);
    for (size_t i = 0; i < n; i++) {
        u64 at, len;
        const int span = hash_item_span(at, len, (const u64*)msg_off, 0, i);
        results[i] = schnorr_verify_lane(mid, sigs + 64 * i, msgs + at, (size_t)len, pks + (pk_format ? 64 : 32) * i, pk_format, span, gtab_host(), g_lm);
    }
    return 1;
}
}
