/* Plain C caller of the engine's C ABI: verify a batch of whitelist signatures that share ONE whitelist
 * (results[i] = what secp256k1_whitelist_signature_parse + secp256k1_whitelist_verify give, include/secp256k1_whitelist.h).
 *
 *   gcc -std=c99 -Iinclude examples/whitelist_verify.c -o whitelist_verify secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./whitelist_verify list.bin items.bin
 * list.bin holds one byte K, then K online keys and K offline keys as 64-byte secp256k1_pubkey objects.
 * items.bin holds, per item: the 64-byte sub key object, then the serialised signature (its first byte says how long it is).
 * Prints one verdict per line; a second batch with one bit of every e0 flipped must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 1024
#define MAX_SIG (1 + 32 * 256)

int main(int argc, char **argv) {
    static unsigned char online[255 * 64], offline[255 * 64], subs[MAX_ITEMS * 64], sigs[MAX_ITEMS * MAX_SIG];
    static uint64_t sig_off[MAX_ITEMS + 1];
    static uint32_t list_of[MAX_ITEMS];
    static int32_t res[MAX_ITEMS];
    uint64_t list_off[2];
    size_t n = 0, i, len;
    int k, c, bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 3) { fprintf(stderr, "usage: %s list.bin items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    k = fgetc(f);
    if (k == EOF || fread(online, 64, (size_t)k, f) != (size_t)k || fread(offline, 64, (size_t)k, f) != (size_t)k) { fprintf(stderr, "%s: truncated\n", argv[1]); fclose(f); return 2; }
    fclose(f);
    list_off[0] = 0; list_off[1] = (uint64_t)k;
    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    sig_off[0] = 0;
    while (n < MAX_ITEMS && fread(subs + 64 * n, 1, 64, f) == 64) {
        if ((c = fgetc(f)) == EOF) { fprintf(stderr, "%s: truncated item %lu\n", argv[2], (unsigned long)n); fclose(f); return 2; }
        len = 32 * ((size_t)c + 1);
        sigs[sig_off[n]] = (unsigned char)c;
        if (fread(sigs + sig_off[n] + 1, 1, len, f) != len) { fprintf(stderr, "%s: truncated item %lu\n", argv[2], (unsigned long)n); fclose(f); return 2; }
        sig_off[n + 1] = sig_off[n] + 1 + len;
        list_of[n] = 0;                                /* every item names list 0: the whitelist goes to the GPU once */
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in res[] */
    if (!secp256k1_whitelist_verify_batch(e, res, sigs, sig_off, online, offline, list_off, 1, list_of, subs, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("%d\n", (int)res[i]);
    for (i = 0; i < n; i++) sigs[sig_off[i] + 1] ^= 1;
    if (!secp256k1_whitelist_verify_batch(e, res, sigs, sig_off, online, offline, list_off, 1, list_of, subs, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 0;
    printf("tampered: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
