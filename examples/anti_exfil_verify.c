/* Plain C caller of the engine's C ABI: the host's side of the ECDSA anti-exfil protocol for a fleet of signing devices.  The host
 * commits to its randomness (what secp256k1_ecdsa_anti_exfil_host_commit writes), and later checks what the devices returned:
 * results[i] = what the parsers + secp256k1_anti_exfil_host_verify give (include/secp256k1_ecdsa_s2c.h), i.e. the signature is valid
 * and its nonce commits to the host's randomness under the device's opening.
 *
 *   gcc -std=c99 -Iinclude examples/anti_exfil_verify.c -o anti_exfil_verify secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./anti_exfil_verify items.bin
 * items.bin holds, per item, 194 bytes: the 64-byte compact signature, the 32-byte message hash, the device's 33-byte compressed
 * public key, the host's 32 bytes of randomness, the device's 33-byte opening.  Prints the host's commitment and both verdicts (the
 * commitment check alone, then the full host verification) per line; then a second batch with one bit of the host's randomness
 * flipped must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 4096

int main(int argc, char **argv) {
    static unsigned char sigs[MAX_ITEMS * 64], msgs[MAX_ITEMS * 32], pks[MAX_ITEMS * 33], rand32[MAX_ITEMS * 32], openings[MAX_ITEMS * 33], commits[MAX_ITEMS * 32];
    static int32_t commit_ok[MAX_ITEMS], host_ok[MAX_ITEMS];
    unsigned char item[194];
    size_t n = 0, i, k;
    int bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_ITEMS && fread(item, 1, 194, f) == 194) {
        memcpy(sigs + 64 * n, item, 64); memcpy(msgs + 32 * n, item + 64, 32); memcpy(pks + 33 * n, item + 96, 33);
        memcpy(rand32 + 32 * n, item + 129, 32); memcpy(openings + 33 * n, item + 161, 33);
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in the result arrays.  sig_format 0: compact signatures (no offsets),
     * pk_format 0 and opening_format 0: compressed keys and openings */
    if (!secp256k1_ecdsa_anti_exfil_host_commit_batch(e, commits, rand32, n) ||
        !secp256k1_ecdsa_s2c_verify_commit_batch(e, commit_ok, sigs, NULL, 0, rand32, openings, 0, n) ||
        !secp256k1_anti_exfil_host_verify_batch(e, host_ok, sigs, NULL, 0, msgs, pks, 0, rand32, openings, 0, n)) {
        fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1;
    }
    for (i = 0; i < n; i++) {
        for (k = 0; k < 32; k++) printf("%02x", commits[32 * i + k]);
        printf(" %d %d\n", (int)commit_ok[i], (int)host_ok[i]);
    }
    for (i = 0; i < n; i++) rand32[32 * i + 31] ^= 1;
    if (!secp256k1_anti_exfil_host_verify_batch(e, host_ok, sigs, NULL, 0, msgs, pks, 0, rand32, openings, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += host_ok[i] != 0;
    printf("randomness bit flipped: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
