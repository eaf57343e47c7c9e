/* Plain C caller of the engine's C ABI: the coordinator of one MuSig2 signing session.  It turns the aggregate nonce, the message and
 * the key-aggregation cache into a session (what secp256k1_musig_nonce_process gives) and checks every signer's share against it (what
 * secp256k1_musig_pubnonce_parse + secp256k1_ec_pubkey_parse + secp256k1_musig_partial_sig_parse + secp256k1_musig_partial_sig_verify
 * give, include/secp256k1_musig.h).  The cache comes from secp256k1_musig_pubkey_agg of the reference: key aggregation runs once per key
 * set and is not served here.
 *
 *   gcc -std=c99 -Iinclude examples/musig_verify.c -o musig_verify secp256k1_zkp_amd/libsecp256k1_zkp_amd.so -Wl,-rpath,$PWD/secp256k1_zkp_amd
 *   ./musig_verify session.bin
 * session.bin holds the 197-byte cache object, the 66-byte serialised aggregate nonce and the 32-byte message, then per signer 131
 * bytes: the 32-byte partial signature, the 66-byte public nonce, the 33-byte compressed public key.  Prints one verdict per line;
 * then a second batch with one bit flipped in every share must come out all 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "secp256k1_zkp_amd.h"

#define MAX_SIGNERS 4096

int main(int argc, char **argv) {
    static unsigned char sigs[MAX_SIGNERS * 32], nonces[MAX_SIGNERS * 66], pks[MAX_SIGNERS * 33];
    static uint32_t session_of[MAX_SIGNERS];                 /* all zero: every share belongs to the one session */
    static int32_t res[MAX_SIGNERS];
    unsigned char cache[197], aggnonce[66], msg[32], session[133], item[131];
    int32_t made = 0;
    size_t n = 0, i;
    int bad = 0;
    FILE *f;
    s2k_engine *e;
    if (argc != 2) { fprintf(stderr, "usage: %s session.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    if (fread(cache, 1, 197, f) != 197 || fread(aggnonce, 1, 66, f) != 66 || fread(msg, 1, 32, f) != 32) { fprintf(stderr, "%s: short file\n", argv[1]); return 2; }
    while (n < MAX_SIGNERS && fread(item, 1, 131, f) == 131) {
        memcpy(sigs + 32 * n, item, 32); memcpy(nonces + 66 * n, item + 32, 66); memcpy(pks + 33 * n, item + 98, 33);
        n++;
    }
    fclose(f);

    e = s2k_engine_create(0);
    if (!e) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    /* the return value is the call's success; the verdict is in made.  nonce_format 0: serialised; no adaptor */
    if (!secp256k1_musig_nonce_process_batch(e, &made, session, aggnonce, 0, msg, cache, NULL, 1)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    if (!made) { fprintf(stderr, "the aggregate nonce or the cache was refused\n"); return 1; }
    /* one cache and one session for all shares; sig_format, nonce_format, pk_format 0: serialised shares, nonces and compressed keys */
    if (!secp256k1_musig_partial_sig_verify_batch(e, res, sigs, 0, nonces, 0, pks, 0, cache, session, 1, session_of, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) printf("%d\n", (int)res[i]);
    for (i = 0; i < n; i++) sigs[32 * i + 31] ^= 1;
    if (!secp256k1_musig_partial_sig_verify_batch(e, res, sigs, 0, nonces, 0, pks, 0, cache, session, 1, session_of, n)) { fprintf(stderr, "engine: %s\n", s2k_last_error()); return 1; }
    for (i = 0; i < n; i++) bad += res[i] != 0;
    printf("share bit flipped: %d accepted\n", bad);
    s2k_engine_destroy(e);
    return bad != 0;
}
