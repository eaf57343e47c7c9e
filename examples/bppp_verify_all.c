/* Plain C caller of the engine's C ABI: one verdict for a whole file of Bulletproofs++ norm arguments over one generator set (what a loop
 * of the reference's per-proof verifier would give when ANDed), and -- only when that verdict is 0 -- which proofs failed.
 *
 *   gcc -std=c99 -Iinclude examples/bppp_verify_all.c -o bppp_verify_all secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./bppp_verify_all batch.bin
 * The file: four little-endian 32-bit words g_len, h_len, proof_len and n; the (g_len + h_len) * 33 bytes of the generator set; then per
 * proof the proof bytes, the 104-byte transcript object, rho (32 bytes), c_vec (h_len * 32 bytes) and the 33-byte commitment.  Prints the
 * verdict, the number of proofs, the seed the batch's coefficients were derived from, and one line per failed proof. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

static size_t le32(const unsigned char *b) { return (size_t)b[0] | ((size_t)b[1] << 8) | ((size_t)b[2] << 16) | ((size_t)b[3] << 24); }

int main(int argc, char **argv) {
    unsigned char head[16], seed[32];
    unsigned char *gens, *proofs, *trs, *rho, *cvec, *commits;
    int32_t verdict = 0, *results;
    size_t g_len, h_len, proof_len, n, i;
    s2k_engine *e;
    FILE *f;
    if (argc != 2) { fprintf(stderr, "usage: %s batch.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    if (fread(head, 1, 16, f) != 16) { fprintf(stderr, "%s: malformed\n", argv[1]); return 2; }
    g_len = le32(head); h_len = le32(head + 4); proof_len = le32(head + 8); n = le32(head + 12);
    if (g_len > 4096 || h_len > 4096 || proof_len > 65536 || n > 65536) { fprintf(stderr, "%s: too large\n", argv[1]); return 2; }
    gens = malloc((g_len + h_len) * 33 + 1); proofs = malloc(n * proof_len + 1); trs = malloc(n * 104 + 1); rho = malloc(n * 32 + 1);
    cvec = malloc(n * h_len * 32 + 1); commits = malloc(n * 33 + 1); results = malloc((n + 1) * sizeof(int32_t));
    if (!gens || !proofs || !trs || !rho || !cvec || !commits || !results) { fprintf(stderr, "out of memory\n"); return 2; }
    if (fread(gens, 33, g_len + h_len, f) != g_len + h_len) { fprintf(stderr, "%s: malformed\n", argv[1]); return 2; }
    for (i = 0; i < n; i++) {
        if (fread(proofs + i * proof_len, 1, proof_len, f) != proof_len || fread(trs + i * 104, 1, 104, f) != 104 || fread(rho + i * 32, 1, 32, f) != 32 ||
            fread(cvec + i * h_len * 32, 32, h_len, f) != h_len || fread(commits + i * 33, 1, 33, f) != 33) { fprintf(stderr, "%s: malformed\n", argv[1]); return 2; }
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdict is written separately.  results may be NULL for a caller that only wants the
     * verdict: the per-proof verifier then never runs. */
    if (!secp256k1_bppp_norm_product_verify_all(e, &verdict, results, seed, proofs, proof_len, trs, rho, gens, g_len + h_len, g_len, cvec, h_len, commits, n)) {
        fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1;
    }
    printf("%d %lu ", (int)verdict, (unsigned long)n);
    for (i = 0; i < 32; i++) printf("%02x", seed[i]);
    printf("\n");
    for (i = 0; i < n; i++) if (!results[i]) printf("invalid: %lu\n", (unsigned long)i);
    s2k_engine_destroy(e);
    free(gens); free(proofs); free(trs); free(rho); free(cvec); free(commits); free(results);
    return 0;
}
