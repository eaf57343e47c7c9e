/* Plain C caller of the engine's C ABI: from the wire bytes of explicit assets and explicit amounts to a balance verdict, as a verifier
 * does for the fee output of every confidential transaction
 * (secp256k1_generator_generate, secp256k1_pedersen_commit with a zero blind, secp256k1_pedersen_verify_tally; include/secp256k1_generator.h).
 *
 *   gcc -std=c99 -Iinclude examples/asset_commit.c -o asset_commit secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./asset_commit items.bin
 * items.bin holds, per item, 48 bytes: a 32-byte asset id, then two 8-byte little-endian numbers; a and b are their top 62 bits plus
 * one (an amount of 0 has no commitment).  Per item the program builds the asset's generator, commits to a, b and a + b with explicit
 * (zero) blinds and checks the tally  C(a) + C(b) - C(a + b) == 0, which must hold, and  C(a) + C(b) - C(a + b + 1) == 0, which must
 * not.  It also round-trips every generator through serialize and parse.
 * Nothing here is constant time: these entry points are for public inputs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 1024

static uint64_t le64(const unsigned char *p) {
    uint64_t v = 0;
    int i;
    for (i = 7; i >= 0; i--) v = (v << 8) | p[i];
    return v;
}

int main(int argc, char **argv) {
    static unsigned char ids[MAX_ITEMS * 32], gens[MAX_ITEMS * 64], gens3[3 * MAX_ITEMS * 64], ser[MAX_ITEMS * 33], back[MAX_ITEMS * 64];
    static unsigned char commits[3 * MAX_ITEMS * 33], tally[2 * 3 * MAX_ITEMS * 33];
    static uint64_t a[MAX_ITEMS], b[MAX_ITEMS], values[3 * MAX_ITEMS], off[2 * MAX_ITEMS + 1], npos[2 * MAX_ITEMS];
    static int32_t res[3 * MAX_ITEMS], verdict[2 * MAX_ITEMS];
    unsigned char item[48];
    size_t n = 0, i;
    int bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_ITEMS && fread(item, 1, 48, f) == 48) {
        memcpy(ids + 32 * n, item, 32); a[n] = le64(item + 32) >> 2; b[n] = le64(item + 40) >> 2;      /* the sums below stay under 2^64 */
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* asset id -> generator object; the return value is the call's success, res[] holds the per-item results */
    if (!secp256k1_generator_generate_batch(e, res, gens, ids, NULL, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 1;
    /* generator object -> 33 wire bytes -> generator object */
    if (!secp256k1_generator_serialize_batch(e, ser, gens, n) || !secp256k1_generator_parse_batch(e, res, back, ser, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 1 || memcmp(back + 64 * i, gens + 64 * i, 64) != 0;
    /* explicit amounts -> commitments: NULL blinds are all-zero blinds */
    for (i = 0; i < n; i++) {
        values[3 * i] = a[i] + 1; values[3 * i + 1] = b[i] + 1; values[3 * i + 2] = a[i] + b[i] + 2;
        memcpy(gens3 + 64 * (3 * i), gens + 64 * i, 64); memcpy(gens3 + 64 * (3 * i + 1), gens + 64 * i, 64); memcpy(gens3 + 64 * (3 * i + 2), gens + 64 * i, 64);
    }
    if (!secp256k1_pedersen_commit_batch(e, res, commits, NULL, values, gens3, 3 * n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < 3 * n; i++) bad += res[i] != 1;
    /* tally 2 i: C(a) + C(b) against C(a + b); tally 2 i + 1: against C(a + b + 1) */
    for (i = 0; i < n; i++) {
        values[i] = a[i] + b[i] + 3;
    }
    if (!secp256k1_pedersen_commit_batch(e, res, ser, NULL, values, gens, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    off[0] = 0;
    for (i = 0; i < n; i++) {
        unsigned char *t0 = tally + 33 * 3 * (2 * i), *t1 = tally + 33 * 3 * (2 * i + 1);
        memcpy(t0, commits + 33 * 3 * i, 99);
        memcpy(t1, commits + 33 * 3 * i, 66); memcpy(t1 + 66, ser + 33 * i, 33);
        npos[2 * i] = npos[2 * i + 1] = 2;
        off[2 * i + 1] = 3 * (2 * i + 1); off[2 * i + 2] = 3 * (2 * i + 2);
    }
    if (!secp256k1_pedersen_verify_tally_batch(e, verdict, tally, off, npos, 2 * n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) {
        printf("%d %d\n", (int)verdict[2 * i], (int)verdict[2 * i + 1]);
        bad += verdict[2 * i] != 1 || verdict[2 * i + 1] != 0;
    }
    printf("unexpected results: %d\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
