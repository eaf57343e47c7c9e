/* Plain C caller of the engine's C ABI: verify a batch of DER-encoded ECDSA signatures against compressed public keys
 * (results[i] = what secp256k1_ecdsa_signature_parse_der + secp256k1_ec_pubkey_parse + secp256k1_ecdsa_verify give, include/secp256k1.h).
 *
 *   gcc -std=c99 -Iinclude examples/ecdsa_verify.c -o ecdsa_verify secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./ecdsa_verify items.bin
 * items.bin holds, per item: one length byte L, L bytes of DER signature, the 32-byte message hash, the 33-byte public key.
 * Prints one verdict per line; a second batch with one bit of every message hash flipped must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 4096

int main(int argc, char **argv) {
    static unsigned char sigs[MAX_ITEMS * 255], msgs[MAX_ITEMS * 32], pks[MAX_ITEMS * 33];
    static uint64_t off[MAX_ITEMS + 1];
    static int32_t res[MAX_ITEMS];
    size_t n = 0, i;
    int c, bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    off[0] = 0;
    while (n < MAX_ITEMS && (c = fgetc(f)) != EOF) {
        if (fread(sigs + off[n], 1, (size_t)c, f) != (size_t)c || fread(msgs + 32 * n, 1, 32, f) != 32 || fread(pks + 33 * n, 1, 33, f) != 33) {
            fprintf(stderr, "%s: truncated item %lu\n", argv[1], (unsigned long)n); fclose(f); return 2;
        }
        off[n + 1] = off[n] + (uint64_t)c;
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in res[] */
    if (!secp256k1_ecdsa_verify_batch(e, res, sigs, off, 2, msgs, pks, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("%d\n", (int)res[i]);
    for (i = 0; i < n; i++) msgs[32 * i + 31] ^= 1;
    if (!secp256k1_ecdsa_verify_batch(e, res, sigs, off, 2, msgs, pks, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 0;
    printf("tampered: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
