/* Plain C caller of the engine's C ABI: sum sets of compressed public keys (nonce sums, input-key sums, key aggregation without
 * coefficients), as secp256k1_ec_pubkey_parse + secp256k1_ec_pubkey_combine + secp256k1_ec_pubkey_serialize do per set
 * (include/secp256k1.h).
 *
 *   gcc -std=c99 -Iinclude examples/pubkey_combine.c -o pubkey_combine secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./pubkey_combine keys.bin 16
 * keys.bin holds 33-byte compressed keys; the second argument is the number of keys per set (the last set takes what is left).
 * The keys are parsed once into objects (one square root each), the objects are combined (the fast path: no root per key) and every
 * sum is printed as a compressed key, or "-" where the set is refused (a key that does not parse, a sum at infinity). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_KEYS 65536

int main(int argc, char **argv) {
    static unsigned char ser[MAX_KEYS * 33], obj[MAX_KEYS * 64], sums[MAX_KEYS * 33];
    static int32_t parsed[MAX_KEYS], res[MAX_KEYS];
    static uint64_t off[MAX_KEYS + 1];
    size_t n = 0, per, n_sets, k, j;
    int refused = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 3 || (per = (size_t)strtoul(argv[2], NULL, 10)) == 0) { fprintf(stderr, "usage: %s keys.bin keys_per_set\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_KEYS && fread(ser + 33 * n, 1, 33, f) == 33) n++;
    fclose(f);
    n_sets = (n + per - 1) / per;
    for (k = 0; k <= n_sets; k++) off[k] = k * per < n ? k * per : n;

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in parsed[] / res[].  A key that does not parse leaves a zero object,
     * which the combine call refuses in turn. */
    if (!secp256k1_ec_pubkey_convert_batch(e, parsed, obj, S2K_PK_OBJECT, NULL, ser, S2K_PK_COMPRESSED, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    if (!secp256k1_ec_pubkey_combine_batch(e, res, sums, S2K_PK_COMPRESSED, NULL, obj, S2K_PK_OBJECT, off, n_sets)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (k = 0; k < n_sets; k++) {
        if (!res[k]) { printf("-\n"); refused++; continue; }
        for (j = 0; j < 33; j++) printf("%02x", sums[33 * k + j]);
        printf("\n");
    }
    s2k_engine_destroy(e);
    return refused != 0;
}
