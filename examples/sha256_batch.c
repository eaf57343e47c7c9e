/* Plain C caller of the engine's C ABI: the double SHA-256 of every line of a file, as Bitcoin's signature hash takes it of its
 * preimages -- the 32-byte msghash32 that secp256k1_ecdsa_verify_batch reads.
 *
 *   gcc -std=c99 -Iinclude examples/sha256_batch.c -o sha256_batch secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./sha256_batch preimages.txt [tag]
 * Every line (without its newline) is one message; the lines lie back to back in one buffer and msg_off says where each starts, so
 * nothing is copied or padded.  With a second argument the digests are tagged hashes instead: secp256k1_tagged_sha256(tag, line). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_BYTES (1u << 24)
#define MAX_ITEMS (1u << 16)

int main(int argc, char **argv) {
    static unsigned char text[MAX_BYTES], out[MAX_ITEMS * 32];
    static uint64_t off[MAX_ITEMS + 1];
    size_t bytes, n = 0, at = 0, i, j, k;
    int ok;
    FILE *f;
    s2k_engine *e;
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: %s preimages.txt [tag]\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    bytes = fread(text, 1, MAX_BYTES, f);
    fclose(f);
    /* the newlines are squeezed out, so that item i is text[off[i] .. off[i+1]) */
    off[0] = 0;
    for (i = 0; i < bytes && n < MAX_ITEMS; i++) {
        if (text[i] == '\n') off[++n] = at; else text[at++] = text[i];
    }
    if (n < MAX_ITEMS && off[n] != at) off[++n] = at;

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    if (argc == 3) ok = secp256k1_tagged_sha256_batch(e, out, (const unsigned char *)argv[2], strlen(argv[2]), text, off, 0, n);
    else ok = s2k_sha256_batch(e, out, text, off, 0, 2, n);
    if (!ok) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (k = 0; k < n; k++) {
        for (j = 0; j < 32; j++) printf("%02x", out[32 * k + j]);
        printf("\n");
    }
    s2k_engine_destroy(e);
    return 0;
}
