// tests/host_emul/hash_batch_bounds.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program for the address and undefined-behaviour sanitizers: the lane routine of csrc/hash_batch.h over messages of
// 0 .. 200 bytes, each in a heap allocation of exactly its length (and the 32-byte output in one of exactly 32), so that a byte read
// outside an item -- the word loads run up to the item's last whole word, the tail is read byte by byte -- is an error the sanitizer
// reports.  Plain, double and tagged; every digest is compared with the byte-at-a-time context of csrc/sha256.h.
// Prints "ok <items>" and returns 0 when all agree.
#include "hash_batch_emu.cpp"
#include <stdio.h>

static void stream_digest(unsigned char* out, int mode, const unsigned char* tag, size_t taglen, const unsigned char* msg, size_t len) {
    sha256_stream h; sha256_stream_init(h);
    if (mode == 2) {
        sha256_stream t; sha256_stream_init(t);
        sha256_stream_write(t, tag, taglen);
        unsigned char th[32]; sha256_stream_finalize(t, th);
        sha256_stream_write(h, th, 32); sha256_stream_write(h, th, 32);
    }
    sha256_stream_write(h, msg, len);
    sha256_stream_finalize(h, out);
    if (mode == 1) {
        sha256_stream g; sha256_stream_init(g);
        sha256_stream_write(g, out, 32);
        sha256_stream_finalize(g, out);
    }
}

int main(void) {
    static const char tag[] = "hash_batch_bounds/tag";
    unsigned items = 0;
    for (size_t len = 0; len <= 200; len++) {
        for (int mode = 0; mode < 3; mode++) {
            unsigned char* msg = new unsigned char[len];                // (length 0: a valid pointer to no bytes)
            for (size_t k = 0; k < len; k++) msg[k] = (unsigned char)(131 * k + 7 * len + mode);
            unsigned char* out = new unsigned char[32];
            unsigned char want[32];
            emu_hash_one(out, mode, (const unsigned char*)tag, sizeof(tag) - 1, msg, len);
            stream_digest(want, mode, (const unsigned char*)tag, sizeof(tag) - 1, msg, len);
            const int bad = memcmp(out, want, 32);
            delete[] msg; delete[] out;
            if (bad) { printf("length %zu mode %d differs\n", len, mode); return 1; }
            items++;
        }
    }
    printf("ok %u\n", items);
    return 0;
}
