/* Plain C caller of the engine's C ABI: one verdict for a whole file of BIP-340 signatures (what a loop of secp256k1_schnorrsig_verify,
 * include/secp256k1_schnorrsig.h, would give when ANDed), and -- only when that verdict is 0 -- which signatures failed.
 *
 *   gcc -std=c99 -Iinclude examples/schnorr_verify_all.c -o schnorr_verify_all secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./schnorr_verify_all items.bin
 * The file holds per signature a 32-byte x-only public key, a 32-byte message and the 64-byte signature.  Prints the verdict, the
 * number of signatures, the seed the batch's coefficients were derived from, and one line per failed signature. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_SIGS 65536

int main(int argc, char **argv) {
    static unsigned char keys[MAX_SIGS * 32], msgs[MAX_SIGS * 32], sigs[MAX_SIGS * 64];
    static int32_t results[MAX_SIGS];
    unsigned char rec[128], seed[32];
    int32_t verdict = 0;
    size_t n = 0, got, i;
    s2k_engine *e;
    FILE *f;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while ((got = fread(rec, 1, 128, f)) == 128 && n < MAX_SIGS) {
        memcpy(keys + 32 * n, rec, 32); memcpy(msgs + 32 * n, rec + 32, 32); memcpy(sigs + 64 * n, rec + 64, 64);
        n++;
    }
    fclose(f);
    if (got != 0) { fprintf(stderr, "%s: malformed or too long\n", argv[1]); return 2; }

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdict is written separately.  msglen 32, pk_format 0: serialised x-only keys.
     * results may be NULL for a caller that only wants the verdict: the per-item verifier then never runs. */
    if (!secp256k1_schnorrsig_verify_all(e, &verdict, results, seed, sigs, msgs, 32, keys, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    printf("%d %lu ", (int)verdict, (unsigned long)n);
    for (i = 0; i < 32; i++) printf("%02x", seed[i]);
    printf("\n");
    for (i = 0; i < n; i++) if (!results[i]) printf("invalid: %lu\n", (unsigned long)i);
    s2k_engine_destroy(e);
    return 0;
}
