// hash_batch.h -- SHA-256 of one message per lane, read as words (s2k_sha256_batch, secp256k1_tagged_sha256_batch; the role of
// secp256k1_sha256_write / _finalize, src/hash_impl.h:145-194, and of secp256k1_tagged_sha256, src/secp256k1.c:869-881).
//
// sha256.h has the compression function and a byte-at-a-time context for cold paths.  Here the message is the hot path: a full block is
// four 16-byte loads and sixteen byte swaps at ANY byte offset (the compiler turns a 16-byte __builtin_memcpy from an unsigned char* into one
// global_load_dwordx4 and __builtin_bswap32 into one v_perm_b32), so there are no alignment cases.  The sixteen message words stay in
// registers: every index into w[] is a compile-time constant, also where the 0x80, the zero fill and the bit length are placed -- the
// word that receives them is chosen by comparing each constant index with the remaining length.
// Reads stay inside [p, p + len): whole words while four bytes remain, then at most three single bytes.  A caller's buffer may end
// with its last item.
// One loop serves every block of a message (data, the block with the 0x80, the block that only carries the length), so a kernel holds
// one copy of the 64 rounds per compression site: the message's and, for the double hash, the second round's.
#pragma once
#include "sha256.h"

struct hash_state { u32 s[8]; };           // a start state: the initial values, or the state behind a 64-byte prefix (the tagged form)

S2K_HD void hash_load4(u32& a, u32& b, u32& c, u32& d, const unsigned char* p) {
    u32 v[4];
    __builtin_memcpy(v, p, 16);
    a = __builtin_bswap32(v[0]); b = __builtin_bswap32(v[1]); c = __builtin_bswap32(v[2]); d = __builtin_bswap32(v[3]);
}
S2K_HD u32 hash_load1(const unsigned char* p) {
    u32 v;
    __builtin_memcpy(&v, p, 4);
    return __builtin_bswap32(v);
}
S2K_HD void hash_store_digest(unsigned char* out32, const u32 s[8]) {
    u32 v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = __builtin_bswap32(s[i]);
    __builtin_memcpy(out32, v, 32);
}

// s <- the state behind the message p[0 .. len) and its padding, started from s with PRE bytes (0 or 64) already absorbed
template <unsigned PRE>
S2K_HD void hash_absorb(u32 s[8], const unsigned char* p, u64 len) {
    static_assert(PRE % 64 == 0, "the prefix is whole blocks");
    const u64 bits = (len + PRE) << 3;
    u64 rem = len;
    u32 pad = 0x80u;                       // 0 once the 0x80 is placed and only the length is left to write
    for (;;) {
        u32 w[16];
        int last = 0;
        if (rem >= 64) {
            hash_load4(w[0], w[1], w[2], w[3], p); hash_load4(w[4], w[5], w[6], w[7], p + 16);
            hash_load4(w[8], w[9], w[10], w[11], p + 32); hash_load4(w[12], w[13], w[14], w[15], p + 48);
            p += 64; rem -= 64;
        } else {
            const u32 r = (u32)rem, nw = r >> 2, t = r & 3;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (r >= 16u * g + 16u) hash_load4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3], p + 16 * g);
                else {
#pragma unroll
                    for (int j = 4 * g; j < 4 * g + 4; j++) w[j] = (u32)j < nw ? hash_load1(p + 4 * j) : 0u;
                }
            }
            // the word behind the whole words: up to three message bytes, then the pad byte
            const unsigned char* q = p + 4 * nw;
            u32 pw = pad << (24 - 8 * t);
            if (t > 0) pw |= (u32)q[0] << 24;
            if (t > 1) pw |= (u32)q[1] << 16;
            if (t > 2) pw |= (u32)q[2] << 8;
#pragma unroll
            for (int j = 0; j < 16; j++) if ((u32)j == nw) w[j] = pw;
            last = r < 56;                 // the length fits behind the pad byte (nw <= 13: words 14 and 15 are zero so far)
            if (last) { w[14] = (u32)(bits >> 32); w[15] = (u32)bits; }
            p += r; rem = 0; pad = 0;
        }
        sha256_compress(s, w);
        if (last) break;
    }
}

// out32 <- SHA256 (SECOND: SHA256(SHA256(.))) of the PRE-byte prefix behind `start` followed by p[0 .. len)
template <unsigned PRE, int SECOND>
S2K_HD void hash_lane(unsigned char* out32, const hash_state& start, const unsigned char* p, u64 len) {
    u32 s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = start.s[i];
    hash_absorb<PRE>(s, p, len);
    if (SECOND) {
        u32 w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = s[i];
        w[8] = 0x80000000u;
#pragma unroll
        for (int i = 9; i < 15; i++) w[i] = 0;
        w[15] = 256;
        sha256_init(s);
        sha256_compress(s, w);
    }
    hash_store_digest(out32, s);
}

// where item i lies: msg_off NULL: [i * msglen, (i + 1) * msglen); else [msg_off[i], msg_off[i + 1]).  0 for a pair of offsets that
// decreases: such an item is answered with zero bytes (verdict 0) and none of its bytes is read.
S2K_HD int hash_item_span(u64& start, u64& len, const u64* msg_off, u64 msglen, size_t i) {
    if (!msg_off) { start = msglen * i; len = msglen; return 1; }
    const u64 a = msg_off[i], b = msg_off[i + 1];
    start = a; len = b - a;
    if (b < a) { start = 0; len = 0; return 0; }
    return 1;
}
// one item of s2k_sha256_batch (PRE 0, start = the initial values) / secp256k1_tagged_sha256_batch (PRE 64, start = the tag's midstate)
template <unsigned PRE, int SECOND>
S2K_HD void hash_batch_item(unsigned char* out32, const hash_state& start, const unsigned char* msgs, const u64* msg_off, u64 msglen, size_t i) {
    u64 at, len;
    if (!hash_item_span(at, len, msg_off, msglen, i)) {
        const u32 z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        __builtin_memcpy(out32 + 32 * i, z, 32);
        return;
    }
    hash_lane<PRE, SECOND>(out32 + 32 * i, start, msgs + at, len);
}
