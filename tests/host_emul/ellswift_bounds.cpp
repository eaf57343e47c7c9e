// tests/host_emul/ellswift_bounds.cpp -- TEST INFRASTRUCTURE ONLY.
// A stand-alone program for the address and undefined-behaviour sanitizers: the lane routines of csrc/ellswift.h over the items of
// tests/golden/ellswift_vectors.json with every input and output in a heap buffer of exactly its documented size (decode: 64 bytes
// in, 32 / 64 / 33 out by format; encode: 64 or 33 bytes of key and 32 of randomness in, 64 out), so that a byte read or written
// outside them is an error the sanitizer reports.  The items come as a flat file the test writes from the golden file:
//   u32 nd, ne, nr (little-endian), then nd records ell64 | object64, ne records key33 | object64 | rnd32 | ell64, nr records
//   format (1 byte) | key (64 bytes, 33 used for format 2).
// Every answer is compared with the recorded one.  Prints "ok <nd> <ne> <nr>" and returns 0 when all agree.
#include "ellswift_emu.cpp"
#include <stdio.h>
#include <vector>

static unsigned char* exact(const unsigned char* src, size_t n) { unsigned char* p = new unsigned char[n]; memcpy(p, src, n); return p; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    unsigned char hdr[12];
    if (fread(hdr, 1, 12, f) != 12) return 2;
    const u32 nd = hdr[0] | (hdr[1] << 8) | (hdr[2] << 16) | ((u32)hdr[3] << 24), ne = hdr[4] | (hdr[5] << 8) | (hdr[6] << 16) | ((u32)hdr[7] << 24),
              nr = hdr[8] | (hdr[9] << 8) | (hdr[10] << 16) | ((u32)hdr[11] << 24);
    if (nd > 100000 || ne > 100000 || nr > 100000) return 2;
    std::vector<unsigned char> rec(193);
    for (u32 i = 0; i < nd; i++) {
        if (fread(rec.data(), 1, 128, f) != 128) return 2;
        const unsigned char* obj = rec.data() + 64;
        unsigned char xbe[32];
        for (int k = 0; k < 32; k++) xbe[k] = obj[31 - k];                     // the object holds x | y as little-endian bytes
        for (int fmt = 0; fmt < 3; fmt++) {
            unsigned char* in = exact(rec.data(), 64);
            const size_t ob = ellswift_out_bytes(fmt);
            unsigned char* out = new unsigned char[ob];
            emu_ellswift_decode(out, fmt, in);
            int bad;
            if (fmt == 0) bad = memcmp(out, xbe, 32);
            else if (fmt == 1) bad = memcmp(out, obj, 64);
            else bad = out[0] != 2 + (obj[32] & 1) || memcmp(out + 1, xbe, 32);
            delete[] in; delete[] out;
            if (bad) { printf("decode item %u format %d differs\n", i, fmt); return 1; }
        }
    }
    for (u32 i = 0; i < ne; i++) {
        if (fread(rec.data(), 1, 193, f) != 193) return 2;
        for (int fmt = 1; fmt <= 2; fmt++) {
            unsigned char* key = fmt == 1 ? exact(rec.data() + 33, 64) : exact(rec.data(), 33);
            unsigned char* rnd = exact(rec.data() + 97, 32);
            unsigned char* out = new unsigned char[64];
            int capped = 0;
            const int r = emu_ellswift_encode(out, &capped, key, fmt, rnd, ELLSWIFT_MAX_ATTEMPTS);
            const int bad = r != 1 || capped || memcmp(out, rec.data() + 129, 64);
            delete[] key; delete[] rnd; delete[] out;
            if (bad) { printf("encode item %u key format %d differs\n", i, fmt); return 1; }
        }
    }
    for (u32 i = 0; i < nr; i++) {
        if (fread(rec.data(), 1, 65, f) != 65) return 2;
        const int fmt = rec[0];
        if (fmt != 1 && fmt != 2) return 2;
        unsigned char* key = exact(rec.data() + 1, fmt == 1 ? 64 : 33);
        unsigned char* rnd = new unsigned char[32]; memset(rnd, 0, 32);
        unsigned char* out = new unsigned char[64]; memset(out, 0xAA, 64);
        int capped = 0, bad;
        bad = emu_ellswift_encode(out, &capped, key, fmt, rnd, ELLSWIFT_MAX_ATTEMPTS) != 0 || capped;
        for (int k = 0; k < 64; k++) bad |= out[k] != 0;
        delete[] key; delete[] rnd; delete[] out;
        if (bad) { printf("refused key %u is not refused\n", i); return 1; }
    }
    fclose(f);
    printf("ok %u %u %u\n", nd, ne, nr);
    return 0;
}
