// tests/host_emul/rp_cached_bases_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// What a generator-cache slot keeps for the rangeproof prologue (csrc/rangeproof.h: rp_gen_chain, rp_gen_y_is_square), compiled for
// the host next to the per-proof routines it stands in for (rp_pp_bases, the square root inside rp_pp_hash).  No fixed-base table needed.
#define S2K_VERIFY 1
#include "../../secp256k1_zkp_amd/csrc/gtable.h"
#include "../../secp256k1_zkp_amd/csrc/sha256.h"
#include "../../secp256k1_zkp_amd/csrc/rangeproof.h"
#include <stdint.h>

extern "C" {
unsigned emu_rp_chain_recs(void) { return RP_CHAIN_RECS; }
unsigned emu_rp_chain_exps(void) { return RP_XMUL_EXPS; }
unsigned emu_rp_gej_words(void) { return RP_GEJ_WORDS; }
// one exponent index of a slot's chain: RP_CHAIN_RECS records (what one lane of k_gen_chain writes)
void emu_rp_gen_chain(uint32_t* chain, const unsigned char* gen64, int exp_idx) { rp_gen_chain(chain, gen64, exp_idx); }
// rp_pp_bases for a parsed proof of `rings` rings and exponent `exp` (-1 .. 18); dbases may be null
void emu_rp_pp_bases(uint32_t* bases, uint32_t* dbases, const unsigned char* gen64, unsigned rings, int exp) {
    rp_rec rec{}; rec.rings = rings; rec.hdr = 1u | ((uint32_t)(exp + 1) << 8);
    rp_pp_bases(rec, bases, gen64, dbases);
}
int emu_rp_gen_y_is_square(const unsigned char* gen64) { return rp_gen_y_is_square(gen64); }
// the message hash of one proof: header parse, then rp_pp_hash with the generator's flag given (0 / 1) or left to the square root (-1).
// Returns whether the header parsed; m: 8 big-endian words.
int emu_rp_hash(uint32_t* m, const unsigned char* commit33, const unsigned char* proof, uint64_t plen, const unsigned char* gen64, int gsq) {
    rp_rec rec{}; u64 mn, mx;
    rp_header(rec, &mn, &mx, proof, plen);
    rp_pp_hash(rec, commit33, proof, nullptr, 0, gen64, gsq);
    for (int i = 0; i < 8; i++) m[i] = rec.m[i];
    return (int)(rec.hdr & 1u);
}
}
