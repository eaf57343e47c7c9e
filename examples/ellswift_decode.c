/* Plain C caller of the engine's C ABI: a BIP-324 listener's side of the handshake for a batch of inbound connections.  Every peer sends
 * a 64-byte ElligatorSwift encoding of its public key; out_i = what secp256k1_ellswift_decode writes for it
 * (include/secp256k1_ellswift.h), here as 33-byte compressed keys.  Then the keys are encoded again with the file's randomness
 * (secp256k1_ellswift_encode; the encodings differ from the inbound ones, an encoding is one of many) and decoded back: every key must
 * come back unchanged.
 *
 *   gcc -std=c99 -Iinclude examples/ellswift_decode.c -o ellswift_decode secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./ellswift_decode items.bin
 * items.bin holds, per item, 96 bytes: the 64-byte encoding and 32 bytes of public randomness.  Prints one compressed key per line,
 * then how many keys did not survive the round trip (0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 4096

int main(int argc, char **argv) {
    static unsigned char ell[MAX_ITEMS * 64], rnd[MAX_ITEMS * 32], keys[MAX_ITEMS * 33], again[MAX_ITEMS * 64], back[MAX_ITEMS * 33];
    static int32_t encoded[MAX_ITEMS];
    unsigned char item[96];
    size_t n = 0, i, k;
    int bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_ITEMS && fread(item, 1, 96, f) == 96) {
        memcpy(ell + 64 * n, item, 64); memcpy(rnd + 32 * n, item + 64, 32);
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; every encoding decodes, so decode has no result array.  out_format 2 and key_format 2:
     * compressed keys */
    if (!secp256k1_ellswift_decode_batch(e, keys, 2, ell, n) ||
        !secp256k1_ellswift_encode_batch(e, encoded, again, keys, 2, rnd, n) ||
        !secp256k1_ellswift_decode_batch(e, back, 2, again, n)) {
        fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1;
    }
    for (i = 0; i < n; i++) {
        for (k = 0; k < 33; k++) printf("%02x", keys[33 * i + k]);
        printf("\n");
        bad += encoded[i] != 1 || memcmp(keys + 33 * i, back + 33 * i, 33) != 0;
    }
    printf("round trip: %d keys lost\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
