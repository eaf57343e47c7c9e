/* Plain C caller of the engine's C ABI: half-aggregate two sets of BIP-340 signatures in one call, then verify both aggregates in one
 * call (what secp256k1_schnorrsig_aggregate and secp256k1_schnorrsig_aggverify give, include/secp256k1_schnorrsig_halfagg.h).
 *
 *   gcc -std=c99 -Iinclude examples/halfagg_batch.c -o halfagg_batch secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./halfagg_batch first.bin second.bin
 * Each file holds one set: per signature a 32-byte x-only public key, a 32-byte message and the 64-byte signature.  Prints per set
 * the verdict of the aggregation, the verdict of the verification and the aggregate's length in bytes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_SIGS 4096

int main(int argc, char **argv) {
    static unsigned char keys[MAX_SIGS * 32], msgs[MAX_SIGS * 32], sigs[MAX_SIGS * 64], aggs[(MAX_SIGS + 2) * 32];
    uint64_t item_off[3] = {0, 0, 0}, aggsig_off[3];
    int32_t made[2], verdict[2];
    size_t n = 0;
    int k;
    s2k_engine *e;
    if (argc != 3) { fprintf(stderr, "usage: %s first.bin second.bin\n", argv[0]); return 2; }
    for (k = 0; k < 2; k++) {
        unsigned char rec[128];
        size_t got;
        FILE *f = fopen(argv[1 + k], "rb");
        if (!f) { perror(argv[1 + k]); return 2; }
        while ((got = fread(rec, 1, 128, f)) == 128 && n < MAX_SIGS) {
            memcpy(keys + 32 * n, rec, 32); memcpy(msgs + 32 * n, rec + 32, 32); memcpy(sigs + 64 * n, rec + 64, 64);
            n++;
        }
        fclose(f);
        if (got != 0) { fprintf(stderr, "%s: malformed or too long\n", argv[1 + k]); return 2; }
        item_off[k + 1] = n;                                 /* set k owns signatures [item_off[k], item_off[k+1]) */
    }

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in made.  pk_format 0: serialised x-only keys.
     * Aggregate k lands at byte 32 (item_off[k] + k) and is 32 (n_k + 1) bytes long: r_0 | ... | r_{n_k - 1} | s */
    if (!secp256k1_schnorrsig_aggregate_batch(e, made, aggs, keys, 0, msgs, sigs, item_off, 2)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (k = 0; k < 3; k++) aggsig_off[k] = 32 * (item_off[k] + (uint64_t)k);
    /* a set that was refused (a key that does not parse) has an all-zero aggregate, which the verifier refuses in turn */
    if (!secp256k1_schnorrsig_aggverify_batch(e, verdict, keys, 0, msgs, item_off, aggs, aggsig_off, 2)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (k = 0; k < 2; k++) printf("%d %d %lu\n", (int)made[k], (int)verdict[k], (unsigned long)(aggsig_off[k + 1] - aggsig_off[k]));
    s2k_engine_destroy(e);
    return 0;
}
