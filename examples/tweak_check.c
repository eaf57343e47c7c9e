/* Plain C caller of the engine's C ABI: check a batch of Taproot commitments, as a script-path spend does once per input
 * (results[i] = what secp256k1_xonly_pubkey_parse + secp256k1_xonly_pubkey_tweak_add_check give, include/secp256k1_extrakeys.h).
 *
 *   gcc -std=c99 -Iinclude examples/tweak_check.c -o tweak_check secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./tweak_check items.bin
 * items.bin holds, per item, 97 bytes: the 32-byte x-only output key, its parity byte, the 32-byte x-only internal key, the 32-byte
 * tweak (the caller's TapTweak hash).  Prints one verdict per line; then the output keys are recomputed from the internal keys and
 * tweaks and compared with the file's, and a second batch with every parity byte flipped must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 4096

int main(int argc, char **argv) {
    static unsigned char out32[MAX_ITEMS * 32], par[MAX_ITEMS], keys[MAX_ITEMS * 32], tweaks[MAX_ITEMS * 32], pk64[MAX_ITEMS * 64];
    static int32_t res[MAX_ITEMS], res2[MAX_ITEMS];
    unsigned char item[97];
    size_t n = 0, i, j;
    int bad = 0, differ = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_ITEMS && fread(item, 1, 97, f) == 97) {
        memcpy(out32 + 32 * n, item, 32); par[n] = item[32]; memcpy(keys + 32 * n, item + 33, 32); memcpy(tweaks + 32 * n, item + 65, 32);
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in res[] */
    if (!secp256k1_xonly_pubkey_tweak_add_check_batch(e, res, out32, par, keys, 0, tweaks, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("%d\n", (int)res[i]);
    /* the add form: secp256k1_pubkey objects, x then y as 32 little-endian bytes each */
    if (!secp256k1_pubkey_tweak_add_batch(e, res2, pk64, keys, 0, tweaks, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) {
        int same = res2[i] && (pk64[64 * i + 32] & 1) == par[i];
        for (j = 0; j < 32; j++) same &= pk64[64 * i + j] == out32[32 * i + 31 - j];
        differ += same != res[i];
    }
    printf("add form disagrees with check form: %d\n", differ);
    for (i = 0; i < n; i++) par[i] ^= 1;
    if (!secp256k1_xonly_pubkey_tweak_add_check_batch(e, res, out32, par, keys, 0, tweaks, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 0;
    printf("parity flipped: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0 || differ != 0;
}
