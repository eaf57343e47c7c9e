/* Plain C caller of the engine's C ABI: verify a batch of ECDSA adaptor signatures, as a party to a discreet-log contract does with the
 * one signature per outcome it receives (results[i] = what secp256k1_ec_pubkey_parse of both keys + secp256k1_ecdsa_adaptor_verify give,
 * include/secp256k1_ecdsa_adaptor.h).
 *
 *   gcc -std=c99 -Iinclude examples/adaptor_verify.c -o adaptor_verify secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./adaptor_verify items.bin
 * items.bin holds, per item, 260 bytes: the 162-byte adaptor signature, the signer's 33-byte compressed public key, the 32-byte
 * message hash, the 33-byte compressed encryption key (the outcome's point).  Prints one verdict per line; then a second batch with
 * one bit flipped in every message must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_ITEMS 4096

int main(int argc, char **argv) {
    static unsigned char sigs[MAX_ITEMS * 162], pks[MAX_ITEMS * 33], msgs[MAX_ITEMS * 32], eks[MAX_ITEMS * 33];
    static int32_t res[MAX_ITEMS];
    unsigned char item[260];
    size_t n = 0, i;
    int bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s items.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    while (n < MAX_ITEMS && fread(item, 1, 260, f) == 260) {
        memcpy(sigs + 162 * n, item, 162); memcpy(pks + 33 * n, item + 162, 33); memcpy(msgs + 32 * n, item + 195, 32); memcpy(eks + 33 * n, item + 227, 33);
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdicts are in res[].  pk_format 0: both key arrays are compressed keys */
    if (!secp256k1_ecdsa_adaptor_verify_batch(e, res, sigs, pks, msgs, eks, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("%d\n", (int)res[i]);
    for (i = 0; i < n; i++) msgs[32 * i + 31] ^= 1;
    if (!secp256k1_ecdsa_adaptor_verify_batch(e, res, sigs, pks, msgs, eks, 0, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 0;
    printf("message bit flipped: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
