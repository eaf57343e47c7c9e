/* secp256k1_zkp_amd.h -- C ABI of the MI355X (gfx950) batch-verification engine.
 *
 * This is the drop-in boundary for the multi-scalar / double-scalar multiplication hot path of
 * BlockstreamResearch/secp256k1-zkp.  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree).  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Conventions (identical to the reference, include/secp256k1.h):
 *   - return 1 = success / valid, 0 = failure / invalid; verification never "errors" on malformed input.
 *   - scalars and field elements are 32-byte big-endian; affine points are 64 bytes x||y big-endian
 *     (the byte layout of `secp256k1_generator`, include/secp256k1_generator.h) with a separate infinity flag.
 *   - the caller owns every buffer; the engine keeps no pointer past a call.
 * Engine-level failures (no device, HIP error) make the *call* return 0 and set s2k_last_error(); a batch that
 * did not complete never reports an item as valid.
 *
 * `_dev` variants take pointers to device (HBM) memory of the engine's GPU and a hipStream_t passed as void*
 * (0 = the engine's own stream); they are asynchronous with respect to the host and are what bench.py times.
 * All device buffers must be 8-byte aligned.
 */
#ifndef SECP256K1_ZKP_AMD_H
#define SECP256K1_ZKP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2K_API __attribute__((visibility("default")))

typedef struct s2k_engine s2k_engine;

/* Create an engine on HIP device `device` (builds the generator table on the GPU).  NULL on failure. */
S2K_API s2k_engine* s2k_engine_create(int device);
S2K_API void s2k_engine_destroy(s2k_engine* e);
/* Last engine-level error of the calling thread ("" if none). */
S2K_API const char* s2k_last_error(void);
/* Why the most recent call on this thread returned 0.  Batch entry points return 0 only for S2K_STATUS_* != OK (verdicts
 * go to results[]); the single-item `_amd` forms return the verdict itself, so for them 0 + S2K_STATUS_OK = "invalid" and
 * 0 + S2K_STATUS_ENGINE_FAILURE = "no verdict: take the CPU path" (a failed engine never yields 1).
 * The `_amd` forms reset the status on entry; batch callers may call s2k_clear_status() first. */
#define S2K_STATUS_OK 0
#define S2K_STATUS_ENGINE_FAILURE 1   /* no device, HIP error, out of memory */
#define S2K_STATUS_ILLEGAL_ARGUMENT 2 /* what the reference's ARG_CHECK would have rejected */
#define S2K_STATUS_BUSY 3             /* both staging sets of the host-buffer rangeproof calls are held by asynchronous tickets */
S2K_API int s2k_last_status(void);
S2K_API void s2k_clear_status(void);
/* Engine options.
 * S2K_OPT_RP_INPUTS_READY (default 0): the rangeproof `_dev` entry points run their first stage (header parse, message hash, ring
 *   bases, commitment lifts: latency bound) on side streams, two calls deep, underneath the previous call's ring kernel.  By default
 *   that stage still waits for everything queued on the caller's stream before the call, because the inputs may be produced there.
 *   Setting the option to 1 is the caller's promise that the input arrays of a `_dev` call are complete when the call is made (and
 *   stay untouched until its results are consumed); min_value/max_value may then be written before the stream reaches the call.
 *   Results are unaffected; host-buffer entry points ignore the option.  An option only: the environment cannot make this promise.
 * S2K_OPT_MSM_PIPELINE (default 0): s2k_ecmult_multi_dev and s2k_ecmult_multi_partial_dev keep TWO calls in flight for small sums (up
 *   to 2^13 terms, where one call is a chain of latency-bound launches): calls alternate between two internal stream / workspace sets
 *   and the caller's stream only waits for each call's result (give calls that may overlap different OUTPUT buffers: results of
 *   consecutive calls are not ordered against each other's writes).  Inputs stay ordered behind the caller's stream unless
 *   S2K_OPT_RP_INPUTS_READY is also set.  Larger sums fill the machine by themselves and run one after the other.
 * S2K_OPT_RP_SPLIT (default 1): two-piece double multiplication in the ring kernel (0: the one-piece form; same results).
 * S2K_OPT_GEN_CACHE_SLOTS (default 2, 0..8; $S2K_GEN_CACHE): how many rangeproof generators may have a fixed-base table at a time
 *   (21.5 GB of HBM each, see s2k_engine_cache_generator).  0 turns the shared-generator form of the ring kernel off.
 * S2K_OPT_GEN_CACHE_MIN (default 65536; $S2K_GEN_CACHE_MIN): an uncached generator gets a table automatically once this many proofs
 *   carrying it have VERIFIED (the last kernel of a call reports them through a device mailbox that the next call reads: junk proofs
 *   that merely name a generator never cost a table).  At most one automatic table is built per call, and it only takes a free slot
 *   or the slot of another automatic table -- never the table of secp256k1_generator_h or one requested through
 *   s2k_engine_cache_generator.
 * S2K_OPT_MAX_LANES (default 2^20, multiples of 256, >= 256): lanes per launch; larger batches run as consecutive sub-range launches.
 * S2K_OPT_STAGE_THREADS (default min(8, cores / 2); $S2K_STAGE_THREADS): host threads that gather a host-buffer rangeproof batch.
 * S2K_OPT_HALFAGG_HOST_CHAIN (default 1): the host-buffer half-aggregate verifier walks the randomizer hash chain on the host
 *   underneath the point-lifting kernel (0: on the device; same verdicts).
 * S2K_OPT_SYNC_SPLIT (default 1): a lone synchronous host-buffer rangeproof call that finds both staging sets free goes as two halves.
 * S2K_OPT_MSM_MAX_TERMS (default 0 = 238 609 293, what 32-bit bucket references index at nine digit windows): s2k_ecmult_multi[_dev] and
 *   s2k_ecmult_multi_partial_dev run a sum with more terms than this as consecutive launches over slices of the term arrays and add the
 *   partial sums -- the reference's own treatment of a sum that exceeds its scratch space (src/ecmult_impl.h:804-820, :856-865).  The
 *   result does not depend on the value; tests lower it to walk the loop at small sizes.
 * S2K_OPT_MUSIG_SUM_FANIN (default 64, 2..64): how many partial points one lane of the MuSig2 summing kernel folds per pass (key and nonce
 *   aggregation).  Results never depend on it; tests lower it to walk the multi-pass loop at small set sizes.
 * S2K_OPT_GTAB_BITS (20, 22, 24 or 26; default 26, $S2K_GTAB_BITS): digit width of the device's fixed-base tables (G and the rangeproof generator
 *   slots: 0.44 / 1.6 / 5.9 / 21.5 GB each, one more addition per fixed-base multiplication for every step down).  Changing it gives the device's
 *   tables back (after a device-wide wait: an administrative call) and the next call that needs one builds it at the new width; a width that
 *   does not fit still falls back to the next narrower one.  Results do not depend on it.
 * S2K_OPT_S2C_FUSED (default 0): secp256k1_anti_exfil_host_verify_batch runs the commitment check and the ECDSA verification in one kernel
 *   instead of the default chain of two (the commitment kernel's verdicts into a byte array, then an ECDSA kernel that ANDs them in).
 *   Results do not depend on it; the chain is the default because it measured faster (tools/s2c_bare.py).
 * S2K_OPT_PUBKEY_FOLD_FANIN (default 16, 2..64): how many keys one lane of the first pass of secp256k1_ec_pubkey_combine_batch folds, and
 *   how many partial sums one lane of its further passes folds.  Every value gives the same results (S2K_OPT_MUSIG_SUM_FANIN does not
 *   touch this call).
 * S2K_OPT_ELLSWIFT_MAX_ATTEMPTS (default and maximum 256, minimum 1): the bound of the rejection loop of secp256k1_ellswift_encode_batch.  An item
 *   that finds no encoding within it gets results[i] = 0 and zero bytes and is counted (s2k_engine_ellswift_capped); at the default this is out
 *   of reach of any input (about 1e-32 per item).  Smaller values exist for tests of the cap; the bytes of an item that succeeds do not depend on it.
 * Environment: only start-up defaults are read from it, once, when an engine (or the device's table pool) is created: S2K_DEVICE,
 * S2K_GEN_CACHE, S2K_GEN_CACHE_MIN, S2K_STAGE_THREADS, S2K_GTAB_BITS.  Nothing on a call path reads the environment. */
#define S2K_OPT_RP_INPUTS_READY 1
#define S2K_OPT_RP_SPLIT 2
#define S2K_OPT_GEN_CACHE_SLOTS 3
#define S2K_OPT_GEN_CACHE_MIN 4
#define S2K_OPT_MSM_PIPELINE 5
#define S2K_OPT_MAX_LANES 6
#define S2K_OPT_STAGE_THREADS 7
#define S2K_OPT_HALFAGG_HOST_CHAIN 8
#define S2K_OPT_SYNC_SPLIT 9
#define S2K_OPT_MSM_MAX_TERMS 10
#define S2K_OPT_GTAB_BITS 11
#define S2K_OPT_MUSIG_SUM_FANIN 12
#define S2K_OPT_S2C_FUSED 13
#define S2K_OPT_ELLSWIFT_MAX_ATTEMPTS 14
#define S2K_OPT_PUBKEY_FOLD_FANIN 15
S2K_API int s2k_engine_set_option(s2k_engine* e, int option, long value);
/* Rangeproof generator tables.  The four public keys of a Borromean ring differ by multiples of the proof's generator
 * (secp256k1_rangeproof_pub_expand, src/modules/rangeproof/rangeproof_impl.h:19-51), so when the engine holds a fixed-base table of that
 * generator a ring builds its odd-multiples tables once instead of four times (~20 % less work per proof).  The table of
 * secp256k1_generator_h (include/secp256k1_generator.h:36) is built at the first rangeproof call; other generators get one through
 * this call (gen64: the 64 bytes of a secp256k1_generator object, host memory) or automatically (S2K_OPT_GEN_CACHE_MIN); the least
 * recently used table makes room ("used" = served proofs that verified, whichever entry point they came through).  Proofs whose generator has no table take the general form of the kernel: results never depend on
 * the cache.  s2k_engine_generator_cached: 1 when gen64 has a table now. */
S2K_API int s2k_engine_cache_generator(s2k_engine* e, const unsigned char* gen64);
S2K_API int s2k_engine_generator_cached(s2k_engine* e, const unsigned char* gen64);
/* Make sure the per-batch HBM workspace can hold `n_items` rangeproofs (optional; calls grow it on demand). */
S2K_API int s2k_engine_reserve(s2k_engine* e, size_t n_items);
/* Block until everything queued on the engine's stream has finished. */
S2K_API int s2k_engine_sync(s2k_engine* e);
/* Device pointer + size (bytes) of the generator table, for tests. */
S2K_API const void* s2k_engine_gtable(s2k_engine* e, size_t* bytes);
/* Digit width D of the device's fixed-base tables (entry (w, v) = v * 2^(D w) * G for the magnitudes v of a signed D-bit digit): 26 =
 * 21.5 GB per table and 10 additions per fixed-base multiplication (the default, $S2K_GTAB_BITS at start-up), 24 / 22 / 20 = 5.9 / 1.6 /
 * 0.44 GB with 11 / 12 / 13 additions.  The first call that needs the table of G allocates the widest one that fits, from the wanted
 * width down, so an engine also exists on a partitioned or shared GPU; rangeproof generator tables take the same width.  Results do not
 * depend on the width.  The reference's knob of this kind is ECMULT_WINDOW_SIZE (src/ecmult.h:14-38). */
S2K_API int s2k_engine_gtable_bits(s2k_engine* e);
/* Device time (ms, HIP events) the construction of the table of G took on this device; negative before the table exists. */
S2K_API float s2k_engine_gtable_build_ms(s2k_engine* e);
/* Wall-clock of the most recent launch group on this engine as measured with hipEvents on its stream (ms);
 * `which`: 0 = whole call, 1 = dominant kernel only; 16 + k = dominant kernel of the k-th most recent rangeproof call (k < 32:
 * several calls may be in flight, see S2K_OPT_RP_INPUTS_READY).  Valid after s2k_engine_sync(). */
S2K_API float s2k_engine_last_ms(s2k_engine* e, int which);
/* 1 if the most recent MSM launch on this engine overflowed a bucket region and took the exact bucket-free path (diagnostics /
 * tests; synchronises the device). */
S2K_API int s2k_engine_last_msm_fallback(s2k_engine* e);
/* Work-list tallies of the most recent rangeproof call on this engine (diagnostics / tests; synchronises the device):
 * out[0] = ring groups the shared-generator form of the rings kernel was given, out[1] = rings the general form processed (its own
 * plus the ones handed back), out[2] = rings handed back because a ring key may be the point at infinity (the reference rejects such a
 * key, src/modules/rangeproof/borromean_impl.h:78), out[3] = rings handed back after an exceptional addition inside a step.
 * (A call of more than two launch groups reports its last two.) */
S2K_API int s2k_engine_rp_handback(s2k_engine* e, uint32_t out[4]);

/* ---- batch double multiplication ---------------------------------------------------------------------------
 * r[i] = na[i]*A[i] + ng[i]*G          replaces: static void secp256k1_ecmult(secp256k1_gej *r,
 *                                       const secp256k1_gej *a, const secp256k1_scalar *na,
 *                                       const secp256k1_scalar *ng)            (src/ecmult.h:47)
 * a_xy: n*64, a_inf: n bytes or NULL (all finite), na: n*32, ng: n*32 or NULL (treated as 0, as the reference's
 * ng == NULL).  Outputs: r_xy n*64 (zeroed when infinite), r_inf n*int32. */
S2K_API int s2k_ecmult_batch(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy,
                             const unsigned char* a_inf, const unsigned char* na, const unsigned char* ng, size_t n);
S2K_API int s2k_ecmult_batch_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy,
                                 const unsigned char* a_inf, const unsigned char* na, const unsigned char* ng, size_t n);
/* r[i] = na[i]*A[i] + nb[i]*B[i]       two variable points, no generator term: what the reference takes two secp256k1_ecmult calls and a
 *                                       secp256k1_gej_add_var for (e.g. src/modules/ecdsa_adaptor/dleq_impl.h:146-150).  The GLV halves
 *                                       of both scalars share one chain of 128 doublings (csrc/ecmult.h: ecmult_lane2); a wavefront
 *                                       with an infinite point, a zero scalar or an exceptional addition takes the two-call form.
 * a_xy, b_xy: n*64; a_inf, b_inf: n bytes or NULL (all finite); na, nb: n*32.  Outputs as s2k_ecmult_batch. */
S2K_API int s2k_ecmult2_batch(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                              const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n);
S2K_API int s2k_ecmult2_batch_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                                  const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n);

/* ---- multi-scalar multiplication ------------------------------------------------------------------------------
 * r = g_sc*G + sum_i sc[i]*pt[i]        replaces: static int secp256k1_ecmult_multi_var(const secp256k1_callback*,
 *                                       secp256k1_scratch*, secp256k1_gej *r, const secp256k1_scalar *inp_g_sc,
 *                                       secp256k1_ecmult_multi_callback cb, void *cbdata, size_t n)
 *                                                                               (src/ecmult.h:62, ecmult_impl.h:823-867)
 * The callback-pull model becomes arrays: sc n*32, pt_xy n*64, pt_inf n bytes or NULL; g_sc 32 bytes or NULL.
 * Entries with sc == 0 or an infinite point are skipped (ecmult_impl.h:523).  Output: r_xy 64 bytes, *r_inf. */
S2K_API int s2k_ecmult_multi(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc,
                             const unsigned char* sc, const unsigned char* pt_xy, const unsigned char* pt_inf, size_t n);
S2K_API int s2k_ecmult_multi_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc,
                                 const unsigned char* sc, const unsigned char* pt_xy, const unsigned char* pt_inf, size_t n);
/* K independent sums in one launch chain: r_k = g_sc_k * G + sum_{i in [offsets[k], offsets[k+1])} sc_i * P_i, k = 0 .. n_sums - 1 -- what a
 * caller of the reference gets from n_sums calls of secp256k1_ecmult_multi_var, e.g. bench_ecmult's 1 024-term sums
 * (src/bench_ecmult.c:262-276, :362-371), one per block or transaction.  ONE small sum is a chain of latency-bound launches (~0.4 ms
 * whatever its size); many of them side by side are binned, accumulated and recombined together (csrc/engine_msm_many.hip), the GPU-natural
 * counterpart of the reference's Strauss-batch regime (src/ecmult_impl.h:382-419).  sc / pt_xy / pt_inf: the sums' terms back to back;
 * offsets: n_sums + 1 increasing term indices starting at 0 -- a HOST array in both forms (read before the call returns); g_sc: n_sums * 32
 * bytes or NULL; r_xy n_sums * 64, r_inf n_sums.  Empty sums give infinity.  Sums of more than 8 192 terms take the single-sum path one
 * after the other. */
S2K_API int s2k_ecmult_multi_many(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc, const unsigned char* sc,
                                  const unsigned char* pt_xy, const unsigned char* pt_inf, const uint64_t* offsets, size_t n_sums);
S2K_API int s2k_ecmult_multi_many_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc, const unsigned char* sc,
                                      const unsigned char* pt_xy, const unsigned char* pt_inf, const uint64_t* offsets_host, size_t n_sums);
/* Partial sums for multi-GPU sharding: writes the Jacobian partial result as 3*9 limbs + flag (28 uint32) so that
 * ranks can all-gather raw limb buffers and finish with s2k_gej_sum (EC addition is not an RCCL op). */
S2K_API int s2k_ecmult_multi_partial_dev(s2k_engine* e, void* stream, uint32_t* r_gej28, const unsigned char* g_sc,
                                         const unsigned char* sc, const unsigned char* pt_xy, const unsigned char* pt_inf, size_t n);
S2K_API int s2k_gej_sum_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const uint32_t* gej28, size_t count);
/* The other way to spread ONE sum over the GPUs of a node (BASELINE config 5: "Pippenger bucket windows sharded across 8 GPUs"):
 * every rank holds all n terms and owns share `part` of `parts` of the signed-digit windows of the bucket method
 * (ecmult_impl.h:516-591 generalised); it returns  sum_{w in share} 2^(c w) S_w  as a Jacobian partial.  The partials of all
 * shares add up to the full result exactly as the term-sharded partials do (all-gather of raw limbs + s2k_gej_sum_dev).
 * All ranks must pass the same n (the window width depends on it) and the same g_sc. */
S2K_API int s2k_ecmult_multi_window_partial_dev(s2k_engine* e, void* stream, uint32_t* r_gej28, const unsigned char* g_sc, const unsigned char* sc,
                                                const unsigned char* pt_xy, const unsigned char* pt_inf, size_t n, uint32_t part, uint32_t parts);

/* ---- BIP-340 batch verification -------------------------------------------------------------------------------
 * results[i] = secp256k1_schnorrsig_verify(ctx, sig64_i, msg_i, msglen, pubkey_i)
 *                                       (include/secp256k1_schnorrsig.h, src/modules/schnorrsig/main_impl.h:215-261)
 * sigs n*64, msgs n*msglen, pubkeys: pk_format 0 = n*32 x-only serialised keys (lifted on the GPU; an invalid key
 * gives 0, as secp256k1_xonly_pubkey_parse would have failed), 1 = n*64 `secp256k1_xonly_pubkey` opaque objects. */
S2K_API int secp256k1_schnorrsig_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const unsigned char* msgs,
                                              size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_schnorrsig_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs,
                                                  const unsigned char* msgs, size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n);

/* ---- ECDSA batch verification -----------------------------------------------------------------------------------
 * results[i] = signature_i parses && public key_i parses && secp256k1_ecdsa_verify(ctx, sig_i, msghash32_i, pubkey_i)
 *                                       (include/secp256k1.h, src/secp256k1.c:498-512, src/ecdsa_impl.h:195-272)
 * As the reference, a signature with s > n/2 is refused (normalise it first).  msghash32 n*32.
 * sig_format 0: sigs n*64 compact r|s big-endian (secp256k1_ecdsa_signature_parse_compact: r or s >= n gives 0);
 *            1: sigs n*64 `secp256k1_ecdsa_signature` opaque objects;
 *            2: DER signatures back to back, item i = sigs[sig_off[i] .. sig_off[i+1]) (sig_off has n+1 entries, as proof_off
 *               of the rangeproof calls), accepted and refused exactly as secp256k1_ecdsa_signature_parse_der does.
 *            sig_off is NULL unless sig_format is 2.
 * pk_format  0: pubkeys n*33 compressed; 1: n*64 `secp256k1_pubkey` opaque objects (an all-zero x, where the reference calls
 *            its illegal-argument callback, gives 0); 2: n*65 uncompressed or hybrid (04 / 06 / 07).  Serialised keys follow
 *            secp256k1_ec_pubkey_parse (src/eckey_impl.h:18-36): an encoding it refuses gives 0. */
S2K_API int secp256k1_ecdsa_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                         const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_ecdsa_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                             int sig_format, const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n);
/* ---- ECDSA public-key recovery ------------------------------------------------------------------------------------
 * results[i] = secp256k1_ecdsa_recover(ctx, &pubkeys_out64[64 i], recoverable signature (sigs64_i, recids[i]), msghash32_i)
 *                                       (include/secp256k1_recovery.h, src/modules/recovery/main_impl.h:87-157)
 * sigs64 n*64 compact r|s; recids n bytes, 0..3 (anything else, like r or s >= n, gives 0, as
 * secp256k1_ecdsa_recoverable_signature_parse_compact would have failed).  pubkeys_out64 n*64: `secp256k1_pubkey` objects
 * (pk_format 1 of the verification calls reads them), 64 zero bytes where results[i] == 0. */
S2K_API int secp256k1_ecdsa_recover_batch(s2k_engine* e, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* sigs64,
                                          const unsigned char* recids, const unsigned char* msghash32, size_t n);
S2K_API int secp256k1_ecdsa_recover_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* sigs64,
                                              const unsigned char* recids, const unsigned char* msghash32, size_t n);

/* ---- ECDSA adaptor-signature batch verification ---------------------------------------------------------------------
 * results[i] = public key_i and encryption key_i parse &&
 *              secp256k1_ecdsa_adaptor_verify(ctx, adaptor_sigs162 + 162 i, pubkey_i, msgs32 + 32 i, enckey_i)
 *                                       (include/secp256k1_ecdsa_adaptor.h, src/modules/ecdsa_adaptor/main_impl.h:236-282;
 *                                        the DLEQ proof: src/modules/ecdsa_adaptor/dleq_impl.h:131-162)
 * adaptor_sigs162 n*162: R | R' | s' | e | s as secp256k1_ecdsa_adaptor_encrypt writes them; msgs32 n*32.  pk_format as in the ECDSA
 * calls (0: n*33 compressed, 1: n*64 `secp256k1_pubkey` objects, an all-zero x giving 0, 2: n*65 uncompressed or hybrid); pubkeys and
 * enckeys share it.  Only verification is served: it reads public data.  Encrypt, decrypt and recover handle secrets and need the
 * reference's constant-time code. */
S2K_API int secp256k1_ecdsa_adaptor_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* adaptor_sigs162, const unsigned char* pubkeys,
                                                 const unsigned char* msgs32, const unsigned char* enckeys, int pk_format, size_t n);
S2K_API int secp256k1_ecdsa_adaptor_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* adaptor_sigs162,
                                                     const unsigned char* pubkeys, const unsigned char* msgs32, const unsigned char* enckeys, int pk_format, size_t n);

/* ---- ECDSA sign-to-contract checks and anti-exfil host verification ----------------------------------------------------
 * verify_commit:  results[i] = signature_i and opening_i parse &&
 *              secp256k1_ecdsa_s2c_verify_commit(ctx, sig_i, data32 + 32 i, opening_i)
 *                                       (include/secp256k1_ecdsa_s2c.h, src/modules/ecdsa_s2c/main_impl.h:88-128;
 *                                        the commitment: secp256k1_ec_commit, src/eccommit_impl.h:48-72)
 * host_verify:    results[i] = signature_i, opening_i and public key_i parse &&
 *              secp256k1_anti_exfil_host_verify(ctx, sig_i, msghash32 + 32 i, pubkey_i, host_data32 + 32 i, opening_i)
 *                                       (src/modules/ecdsa_s2c/main_impl.h:185-188: verify_commit, then secp256k1_ecdsa_verify)
 * host_commit:    commitments_out32 + 32 i = what secp256k1_ecdsa_anti_exfil_host_commit(ctx, ., rand32 + 32 i) writes (:131-144)
 * sigs, sig_off, sig_format, pubkeys and pk_format mean what they mean in secp256k1_ecdsa_verify_batch (with DER, sig_off is a host
 * array in the host and group forms and a device array in the _dev forms).  The commitment check reads r alone: a high or zero s passes
 * it and fails host_verify.  openings: opening_format 0: n*33 compressed, as secp256k1_ecdsa_s2c_opening_parse reads them;
 * 1: n*64 `secp256k1_ecdsa_s2c_opening` objects, which have the layout of `secp256k1_pubkey` (an all-zero x gives 0).
 * Only the host's and the auditor's side is served: it reads public data.  secp256k1_ecdsa_s2c_sign, secp256k1_ecdsa_anti_exfil_signer_commit
 * and secp256k1_anti_exfil_sign handle secrets and need the reference's constant-time code. */
S2K_API int secp256k1_ecdsa_s2c_verify_commit_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                    const unsigned char* data32, const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_ecdsa_s2c_verify_commit_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                        int sig_format, const unsigned char* data32, const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_anti_exfil_host_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                   const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, const unsigned char* host_data32,
                                                   const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_anti_exfil_host_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                       int sig_format, const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format,
                                                       const unsigned char* host_data32, const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_ecdsa_anti_exfil_host_commit_batch(s2k_engine* e, unsigned char* commitments_out32, const unsigned char* rand32, size_t n);
S2K_API int secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(s2k_engine* e, void* stream, unsigned char* commitments_out32, const unsigned char* rand32, size_t n);

/* ---- ElligatorSwift (BIP-324): batch decoding and encoding of public keys ------------------------------------------------
 * decode:  out_i = what secp256k1_ellswift_decode(ctx, ., ell64 + 64 i) writes
 *                                       (include/secp256k1_ellswift.h, src/modules/ellswift/main_impl.h:470-483; the map:
 *                                        secp256k1_ellswift_xswiftec_frac_var :24-132)
 *          out_format 0: n*32, ser32(x) alone (secp256k1_ellswift_xswiftec_var :135-140; no root for y is taken)
 *                     1: n*64 secp256k1_pubkey objects, byte for byte the reference's
 *                     2: n*33 compressed keys (what secp256k1_ec_pubkey_serialize makes of those objects)
 *          Every 64 bytes decode (u and t >= p are reduced, not refused), so there is no results array and the call returns 1.
 * encode:  results[i], ell64_out + 64 i = what the key parser + secp256k1_ellswift_encode(ctx, ., key_i, rnd32 + 32 i) give
 *                                       (src/modules/ellswift/main_impl.h:393-420; the loop: :333-382; the partial inverse: :168-303)
 *          key_format 1: n*64 secp256k1_pubkey objects; 2: n*33 compressed keys, accepted and refused as secp256k1_ec_pubkey_parse does.
 *          results[i] = 0 and 64 zero bytes for a refused key and for the all-zero object (the reference: illegal-argument callback,
 *          0, zeros); the neighbours are not affected.  rnd32 is PUBLIC randomness: nothing here is constant time.
 *          The one deviation from the reference: its loop runs until it succeeds, the engine's stops after 256 attempts
 *          (S2K_OPT_ELLSWIFT_MAX_ATTEMPTS; about 1/4 of the attempts succeed, so no input gets there: (3/4)^256 ~ 1e-32).  Such an item
 *          gets results[i] = 0 and zero bytes, and s2k_engine_ellswift_capped() counts it.
 * NULL where the reference has ARG_CHECK, or a format out of range, is S2K_STATUS_ILLEGAL_ARGUMENT (return 0); n == 0 returns 1.  The
 * _dev forms take device pointers and zero their outputs on the stream first.
 * secp256k1_ellswift_create and secp256k1_ellswift_xdh handle a secret key and need the reference's constant-time code. */
S2K_API int secp256k1_ellswift_decode_batch(s2k_engine* e, unsigned char* out, int out_format, const unsigned char* ell64, size_t n);
S2K_API int secp256k1_ellswift_decode_batch_dev(s2k_engine* e, void* stream, unsigned char* out, int out_format, const unsigned char* ell64, size_t n);
S2K_API int secp256k1_ellswift_encode_batch(s2k_engine* e, int32_t* results, unsigned char* ell64_out, const unsigned char* keys, int key_format,
                                            const unsigned char* rnd32, size_t n);
S2K_API int secp256k1_ellswift_encode_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* ell64_out, const unsigned char* keys, int key_format,
                                                const unsigned char* rnd32, size_t n);
/* *count = the items of this engine's encode calls that have hit the attempt cap since the engine was created.  Waits for the device. */
S2K_API int s2k_engine_ellswift_capped(s2k_engine* e, uint64_t* count);

/* ---- MuSig2: batch partial-signature verification and nonce processing (the coordinator's half) ------------------------
 * results[i] = inputs parse &&
 *              secp256k1_musig_partial_sig_verify(ctx, sig_i, pubnonce_i, pubkey_i, cache_S, session_S),   S = session_of[i]
 *                                       (include/secp256k1_musig.h, src/modules/musig/session_impl.h:716-777)
 * partial_sigs   sig_format 0: n*32 serialised (a value >= the group order is refused, as secp256k1_musig_partial_sig_parse);
 *                1: n*36 `secp256k1_musig_partial_sig` objects (the scalar is reduced, not refused).
 * pubnonces      nonce_format 0: n*66 serialised as secp256k1_musig_pubnonce_parse reads them (two compressed points; 33 zero bytes
 *                are NOT accepted); 1: n*132 `secp256k1_musig_pubnonce` objects.
 * pubkeys        pk_format as in the ECDSA calls (0: n*33, 1: n*64 `secp256k1_pubkey` objects, 2: n*65).
 * keyagg_caches197, sessions133: n_sessions `secp256k1_musig_keyagg_cache` and `secp256k1_musig_session` objects, one pair per
 *                signing session; session_of[i] names the pair of share i, so a session with many signers is uploaded once.
 *                session_of NULL: n_sessions == n and share i uses pair i.
 * The host and group forms fail with S2K_STATUS_ILLEGAL_ARGUMENT when some session_of[i] >= n_sessions; in the _dev form, where
 * session_of is device memory like every other array, that share gets verdict 0.  The session's s part and final nonce are not read.
 * Points inside objects are read as they are: an off-curve point is the caller's error and stays with its item.
 * DIFFERENCE FROM THE REFERENCE: where secp256k1_musig_partial_sig_verify calls the illegal-argument callback (a wrong magic in any
 * of the four objects, an all-zero key object) the item gets verdict 0 and its neighbours are unaffected.
 *
 * results[i] = inputs parse &&
 *              secp256k1_musig_nonce_process(ctx, sessions_out133 + 133 i, aggnonce_i, msgs32 + 32 i, cache_i, adaptor_i or NULL)
 *                                       (session_impl.h:588-638)
 * aggnonces      nonce_format 0: n*66 serialised as secp256k1_musig_aggnonce_parse reads them (33 zero bytes: infinity);
 *                1: n*132 `secp256k1_musig_aggnonce` objects.
 * keyagg_caches197 n*197; adaptors64 NULL (no item has an adaptor) or n*64 `secp256k1_pubkey` objects.
 * sessions_out133 matches `secp256k1_musig_session` byte for byte and feeds the verifier above, in the _dev forms without leaving
 * device memory.  DIFFERENCE FROM THE REFERENCE: where results[i] == 0 the session is 133 zero bytes; the reference leaves the
 * object untouched there (and calls the illegal-argument callback on a wrong magic or an all-zero adaptor object).
 *
 * Out of scope, with the reference: everything that touches a secret (nonce_gen*, partial_sign, adapt, extract_adaptor).  Key
 * aggregation, the cache tweaks, nonce aggregation and signature aggregation are the next section. */
S2K_API int secp256k1_musig_partial_sig_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* partial_sigs, int sig_format,
                                                     const unsigned char* pubnonces, int nonce_format, const unsigned char* pubkeys, int pk_format,
                                                     const unsigned char* keyagg_caches197, const unsigned char* sessions133, size_t n_sessions,
                                                     const uint32_t* session_of, size_t n);
S2K_API int secp256k1_musig_partial_sig_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* partial_sigs, int sig_format,
                                                         const unsigned char* pubnonces, int nonce_format, const unsigned char* pubkeys, int pk_format,
                                                         const unsigned char* keyagg_caches197, const unsigned char* sessions133, size_t n_sessions,
                                                         const uint32_t* session_of, size_t n);
S2K_API int secp256k1_musig_nonce_process_batch(s2k_engine* e, int32_t* results, unsigned char* sessions_out133, const unsigned char* aggnonces,
                                                int nonce_format, const unsigned char* msgs32, const unsigned char* keyagg_caches197,
                                                const unsigned char* adaptors64, size_t n);
S2K_API int secp256k1_musig_nonce_process_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* sessions_out133, const unsigned char* aggnonces,
                                                    int nonce_format, const unsigned char* msgs32, const unsigned char* keyagg_caches197,
                                                    const unsigned char* adaptors64, size_t n);

/* ---- MuSig2: key aggregation, cache tweaks, nonce aggregation, signature aggregation (the rest of the coordinator's flow) -----
 * With the two calls above a signing round stays on the device: keys -> cache -> tweaked cache -> aggregate nonce -> session ->
 * share verdicts -> final BIP-340 signature (which secp256k1_schnorrsig_verify_batch_dev can check on the spot).  All public data.
 * Conventions as above: results[] per item; 0 and zeroed outputs for a refused item, neighbours never affected;
 * S2K_STATUS_ILLEGAL_ARGUMENT only for NULL arguments, out-of-range formats and offsets that do not start at 0 or that decrease.  In
 * the _dev forms every byte array is in HBM, outputs and results are zeroed on the stream first, and the offset arrays are HOST
 * arrays of n + 1 entries, read before the call returns (as offsets_host of s2k_ecmult_multi_many_dev).
 *
 * results[k] = secp256k1_musig_pubkey_agg(ctx, agg_pks_out64 + 64 k, caches_out197 + 197 k, keys of set k, set_off[k+1] - set_off[k])
 *                                       (src/modules/musig/keyagg_impl.h:156-215)
 * pubkeys        the keys of all sets, one after the other; set k owns keys [set_off[k], set_off[k+1]).  pk_format as in the ECDSA
 *                calls (0: 33 bytes each, 1: 64-byte `secp256k1_pubkey` objects, 2: 65 bytes uncompressed or hybrid).
 * caches_out197  byte for byte `secp256k1_musig_keyagg_cache`: magic | pk | second_pk (64 zero bytes when every key equals the first)
 *                | pks_hash | parity_acc 0 | tweak 0.  agg_pks_out64 (may be NULL): the `secp256k1_xonly_pubkey` object (even y).
 * The second key is the first key that differs from key 0: format 1 compares the 64 bytes (the reference's memcmp), format 0 the 33
 * bytes, format 2 bytes 1..64, so that a hybrid encoding of key 0's point is NOT a second key.
 * results[k] == 0 with zeroed outputs: an empty set (the reference: ARG_CHECK(n_pubkeys > 0)); a set with a key that does not parse
 * or an all-zero-x object; DIFFERENCE FROM THE REFERENCE: an aggregate at infinity, which no hash reaches and the reference only
 * guards with a VERIFY_CHECK.
 *
 * results[i] = xonly[i] ? secp256k1_musig_pubkey_xonly_tweak_add(ctx, pubkeys_out64 + 64 i, cache_i, tweaks32 + 32 i)
 *                       : secp256k1_musig_pubkey_ec_tweak_add(...)        (keyagg_impl.h:231-273)
 * xonly NULL: every item is a plain tweak; a byte other than 0 or 1 gives 0.  caches_out197 may be the very buffer caches_in197 (the
 * reference works in place); any other overlap is not supported.  pubkeys_out64 (may be NULL): `secp256k1_pubkey` objects.
 * A host-form call that fails as a whole (return 0) leaves zeroed outputs, except the caches of an in-place call, which are its input.
 * results[i] == 0: a wrong cache magic, a tweak >= the group order, a result at infinity.  DIFFERENCE FROM THE REFERENCE: the output
 * cache is then 197 zero bytes; the reference leaves the cache as it was.
 *
 * results[k] = pubnonces parse && secp256k1_musig_nonce_agg(ctx, aggnonce_k, pubnonces of session k, nonce_off[k+1] - nonce_off[k])
 *                                       (session_impl.h:493-531)
 * pubnonces      nonce_format 0: 66 bytes each as secp256k1_musig_pubnonce_parse reads them; 1: 132-byte objects.
 * aggnonces_out  out_format 0: 66 bytes each as secp256k1_musig_aggnonce_serialize writes them; 1: 132-byte `secp256k1_musig_aggnonce`
 *                objects.  An infinite sum is a valid result: 33 zero bytes serialised, 64 zero bytes inside the object.
 * results[k] == 0 with zeroed output: an empty range, a wrong pubnonce magic, a serialised pubnonce the parser refuses (33 zero bytes
 * included).
 *
 * results[k] = shares parse && secp256k1_musig_partial_sig_agg(ctx, sigs64_out + 64 k, session_k, shares of session k, ...)
 *                                       (session_impl.h:779-805)
 * sigs64_out     fin_nonce | (s_part + sum of s_i) mod n: the BIP-340 signature.  partial_sigs: sig_format as in the verifier.
 * results[k] == 0 with 64 zero bytes: an empty range, a wrong session or signature magic, a serialised s >= n (an object holding
 * s = n is reduced, not refused, as in the verifier).
 *
 * Out of scope: group forms of these four calls, the hook into the reference's own functions (integration/), pubkey_get (bytes 4..67
 * of the cache are the key) and BIP-328 derivation; and, as above, everything that touches a secret. */
S2K_API int secp256k1_musig_pubkey_agg_batch(s2k_engine* e, int32_t* results, unsigned char* caches_out197, unsigned char* agg_pks_out64, const unsigned char* pubkeys,
                                             int pk_format, const uint64_t* set_off, size_t n_sets);
S2K_API int secp256k1_musig_pubkey_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* caches_out197, unsigned char* agg_pks_out64,
                                                 const unsigned char* pubkeys, int pk_format, const uint64_t* set_off, size_t n_sets);
S2K_API int secp256k1_musig_pubkey_tweak_add_batch(s2k_engine* e, int32_t* results, unsigned char* caches_out197, unsigned char* pubkeys_out64,
                                                   const unsigned char* caches_in197, const unsigned char* tweaks32, const unsigned char* xonly, size_t n);
S2K_API int secp256k1_musig_pubkey_tweak_add_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* caches_out197, unsigned char* pubkeys_out64,
                                                       const unsigned char* caches_in197, const unsigned char* tweaks32, const unsigned char* xonly, size_t n);
S2K_API int secp256k1_musig_nonce_agg_batch(s2k_engine* e, int32_t* results, unsigned char* aggnonces_out, int out_format, const unsigned char* pubnonces,
                                            int nonce_format, const uint64_t* nonce_off, size_t n_sessions);
S2K_API int secp256k1_musig_nonce_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggnonces_out, int out_format,
                                                const unsigned char* pubnonces, int nonce_format, const uint64_t* nonce_off, size_t n_sessions);
S2K_API int secp256k1_musig_partial_sig_agg_batch(s2k_engine* e, int32_t* results, unsigned char* sigs64_out, const unsigned char* sessions133,
                                                  const unsigned char* partial_sigs, int sig_format, const uint64_t* sig_off, size_t n_sessions);
S2K_API int secp256k1_musig_partial_sig_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* sigs64_out, const unsigned char* sessions133,
                                                      const unsigned char* partial_sigs, int sig_format, const uint64_t* sig_off, size_t n_sessions);

/* ---- Whitelist-signature batch verification -------------------------------------------------------------------------
 * results[i] = secp256k1_whitelist_signature_parse(ctx, &sig, sigs + sig_off[i], sig_off[i+1] - sig_off[i]) &&
 *              secp256k1_whitelist_verify(ctx, &sig, online keys of list L, offline keys of list L, length of list L, sub64 + 64 i),   L = list_of[i]
 *                                       (include/secp256k1_whitelist.h, src/modules/whitelist/main_impl.h:99-151)
 * sigs: serialised signatures back to back (n_keys byte | e0 | s_0 .. s_{n_keys-1}), item i = sigs[sig_off[i] .. sig_off[i+1]).
 * online64 / offline64: the key lists back to back, 64-byte `secp256k1_pubkey` opaque objects; list l owns keys
 * [list_off[l], list_off[l+1]); list_off has n_lists + 1 non-decreasing entries starting at 0.  list_of[i] names item i's list;
 * NULL means n_lists == n and item i uses list i.  A whitelist shared by the whole batch is therefore uploaded once.
 * sub64 n*64: one `secp256k1_pubkey` object per item.
 * An item whose list is longer than 255 keys, or whose signature is not 1 + 32 (list length + 1) bytes long, gets verdict 0 (not a
 * call error) and costs no key work.  An all-zero key object, where the reference calls its illegal-argument callback and then
 * reads an unset point, gives the item 0.  list_of[i] >= n_lists, decreasing offsets and NULL where the reference has ARG_CHECK
 * are S2K_STATUS_ILLEGAL_ARGUMENT (return 0, results zeroed).
 * _dev: the byte arrays and results are in HBM; the three offset / index arrays are HOST arrays, read before the call returns (as
 * offsets_host of s2k_ecmult_multi_many_dev): the call plans its launches from them.  results is zeroed on the stream first. */
S2K_API int secp256k1_whitelist_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                             const unsigned char* online64, const unsigned char* offline64, const uint64_t* list_off, size_t n_lists,
                                             const uint32_t* list_of, const unsigned char* sub64, size_t n);
S2K_API int secp256k1_whitelist_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off_host,
                                                 const unsigned char* online64, const unsigned char* offline64, const uint64_t* list_off_host, size_t n_lists,
                                                 const uint32_t* list_of_host, const unsigned char* sub64, size_t n);

/* ---- Taproot tweak checks ------------------------------------------------------------------------------------------
 * results[i] = secp256k1_xonly_pubkey_tweak_add_check(ctx, tweaked32_i, parities[i], internal_i, tweak32_i)
 *                                       (include/secp256k1_extrakeys.h, src/modules/extrakeys/main_impl.h:135-154)
 * tweaked32 n*32: the serialised x-only output keys; parities n bytes (anything other than 0 or 1 gives 0: the reference compares
 * the int); tweaks32 n*32 big-endian (>= n gives 0; 0 is legal and leaves the key as it is).
 * key_format 0: internal_keys n*32 serialised x-only keys, accepted and refused as secp256k1_xonly_pubkey_parse does
 *               (extrakeys/main_impl.h:22-42);
 *            1: internal_keys n*64 `secp256k1_xonly_pubkey` opaque objects, read as they are (an all-zero object, where the
 *               reference calls its illegal-argument callback, gives 0).
 * NULL where the reference has ARG_CHECK or a key_format out of range is S2K_STATUS_ILLEGAL_ARGUMENT (return 0).
 * _dev: every array in HBM; results is zeroed on the stream first. */
S2K_API int secp256k1_xonly_pubkey_tweak_add_check_batch(s2k_engine* e, int32_t* results, const unsigned char* tweaked32, const unsigned char* parities,
                                                         const unsigned char* internal_keys, int key_format, const unsigned char* tweaks32, size_t n);
S2K_API int secp256k1_xonly_pubkey_tweak_add_check_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* tweaked32,
                                                             const unsigned char* parities, const unsigned char* internal_keys, int key_format,
                                                             const unsigned char* tweaks32, size_t n);
/* ---- public-key tweak-add -------------------------------------------------------------------------------------------
 * results[i] = secp256k1_xonly_pubkey_tweak_add(ctx, &pubkeys_out64[64 i], key_i, tweak32_i)     (key_format 0, 1)
 *                                       (include/secp256k1_extrakeys.h, src/modules/extrakeys/main_impl.h:118-133)
 *            = secp256k1_ec_pubkey_tweak_add(ctx, key_i -> &pubkeys_out64[64 i], tweak32_i)      (key_format 1, 2)
 *                                       (include/secp256k1.h, src/secp256k1.c:766-790, src/eckey_impl.h:62-72)
 * key_format 0 and 1 as above (1 is also the `secp256k1_pubkey` object: both load identically); 2: keys n*33 compressed keys,
 * accepted and refused as secp256k1_ec_pubkey_parse does.  pubkeys_out64 n*64: `secp256k1_pubkey` objects, 64 zero bytes where
 * results[i] == 0 (key refused, tweak >= n, or key + tweak G is the point at infinity).
 * _dev: every array in HBM; results and pubkeys_out64 are zeroed on the stream first. */
S2K_API int secp256k1_pubkey_tweak_add_batch(s2k_engine* e, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* keys, int key_format,
                                             const unsigned char* tweaks32, size_t n);
S2K_API int secp256k1_pubkey_tweak_add_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* keys,
                                                 int key_format, const unsigned char* tweaks32, size_t n);

/* ---- public keys: conversion between encodings, negation, tweak-mul, combine ---------------------------------------------
 * PUBLIC INPUTS ONLY: nothing below is constant time.  The engine uses five encodings of a curve point; these calls move a batch
 * from any of them to any other without leaving HBM, and serve the public-key group of include/secp256k1.h.
 *   S2K_PK_XONLY        32 bytes   in: as secp256k1_xonly_pubkey_parse (src/modules/extrakeys/main_impl.h:22-42: x >= p or x not on
 *                                  the curve gives 0; the even y).  out: ser32(x) (secp256k1_xonly_pubkey_serialize behind
 *                                  secp256k1_xonly_pubkey_from_pubkey, :44-59, :85-116)
 *   S2K_PK_OBJECT       64 bytes   the opaque `secp256k1_pubkey` / `secp256k1_xonly_pubkey` object.  in: read as it is
 *                                  (secp256k1_pubkey_load; an odd y stays odd).  out: byte for byte what secp256k1_pubkey_save writes
 *   S2K_PK_COMPRESSED   33 bytes   in: secp256k1_ec_pubkey_parse, 33-byte case (src/secp256k1.c:290-306, src/eckey_impl.h:18-36).
 *                                  out: secp256k1_ec_pubkey_serialize(.., SECP256K1_EC_COMPRESSED) (secp256k1.c:308-332)
 *   S2K_PK_FULL         65 bytes   in: secp256k1_ec_pubkey_parse, 65-byte case: prefixes 04 / 06 / 07 with the hybrid parity rule.
 *                                  out: prefix 04 (SECP256K1_EC_UNCOMPRESSED)
 *   S2K_PK_AFFINE       64 bytes   x | y big-endian: a_xy / pt_xy / r_xy of s2k_ecmult_batch, s2k_ecmult2_batch, s2k_ecmult_multi*.
 *                                  in: accepted iff x < p, y < p and the point is on the curve.  out: x | y
 *   S2K_PK_XONLY_OBJECT 64 bytes   OUTPUT ONLY (as input it is S2K_PK_OBJECT): the object with y made even
 *                                  (secp256k1_xonly_pubkey_from_pubkey)
 * (0, 1 and 2 are the key_format numbers of the tweak calls above.)  Formats 0 and 2 cost a square root per key on the way in, 3 and 4
 * an on-curve check, 1 nothing.
 * Common to every call: results[i] is the reference's return value; where it is 0 the item's output bytes are all zero.  parities_out
 * (n bytes, may be NULL) receives is_odd(y) of the result point -- for the two x-only output formats that is the parity the encoding
 * drops, the pk_parity of secp256k1_xonly_pubkey_from_pubkey -- and 0 where the item is refused.  n == 0 returns 1; NULL where the
 * reference has ARG_CHECK or a format out of range is S2K_STATUS_ILLEGAL_ARGUMENT (return 0).  The host forms zero results and the
 * outputs before anything can fail; the _dev forms (every array in HBM) zero them on the stream first.
 * DIFFERENCES FROM THE REFERENCE: S2K_PK_AFFINE is defined here (the reference has no such call); a refused item's output is zero
 * bytes in EVERY output format (the reference's serialisers leave their buffer's tail as it was); an object whose x is all zero,
 * where the reference calls its illegal-argument callback, gives 0.
 *
 * convert:   out_i = in_i in another encoding.  By choice of formats: secp256k1_ec_pubkey_parse (2 or 3 -> 1),
 *            secp256k1_ec_pubkey_serialize (1 -> 2 or 3), secp256k1_xonly_pubkey_parse (0 -> 1), secp256k1_xonly_pubkey_serialize
 *            (1 -> 0), secp256k1_xonly_pubkey_from_pubkey (1 -> 5, with parities_out), and the bridge to and from x | y (4).
 * negate:    the same with y negated before the store (secp256k1_ec_pubkey_negate, secp256k1.c:723-736). */
#define S2K_PK_XONLY 0
#define S2K_PK_OBJECT 1
#define S2K_PK_COMPRESSED 2
#define S2K_PK_FULL 3
#define S2K_PK_AFFINE 4
#define S2K_PK_XONLY_OBJECT 5
S2K_API int secp256k1_ec_pubkey_convert_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                              const unsigned char* in, int in_format, size_t n);
S2K_API int secp256k1_ec_pubkey_convert_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                  const unsigned char* in, int in_format, size_t n);
S2K_API int secp256k1_ec_pubkey_negate_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                             const unsigned char* in, int in_format, size_t n);
S2K_API int secp256k1_ec_pubkey_negate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                 const unsigned char* in, int in_format, size_t n);
/* tweak-mul: results[i] = secp256k1_ec_pubkey_tweak_mul(ctx, key_i -> out_i, tweak32_i)      (secp256k1.c:810-831, eckey_impl.h:82-92)
 * 0 for a tweak >= the group order, a tweak of 0 and a key that does not load; otherwise out_i = t_i * P_i, which is never infinite.
 * tweaks32 n*32 big-endian.  One variable-point multiplication per item: the cost of s2k_ecmult_batch with ng == NULL. */
S2K_API int secp256k1_ec_pubkey_tweak_mul_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                const unsigned char* keys, int key_format, const unsigned char* tweaks32, size_t n);
S2K_API int secp256k1_ec_pubkey_tweak_mul_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                    const unsigned char* keys, int key_format, const unsigned char* tweaks32, size_t n);
/* combine: results[k] = secp256k1_ec_pubkey_combine(ctx, out_k, the keys of set k, their count)      (secp256k1.c:843-867)
 * keys: the keys of all sets, concatenated; set k owns keys [key_off[k], key_off[k+1]).  key_off has n_sets + 1 entries, starts at 0,
 * never decreases and is a HOST array in both forms, read before the call returns.  0 for an empty set (ARG_CHECK(n >= 1)), a set with a
 * key that does not load (DIFFERENCE: the reference ignores secp256k1_pubkey_load's verdict there after its callback) and a sum at
 * infinity; otherwise the sum.  A launch chain planned from the offsets: a first pass in which one lane folds up to F consecutive keys
 * of one set straight from their bytes (S2K_OPT_PUBKEY_FOLD_FANIN), further passes only while a set has more than one partial sum, one
 * to-affine step per set.  Keys in formats 0 and 2 cost a square root EACH (they are first loaded one key per lane, so that the roots
 * run side by side, and then summed): S2K_PK_OBJECT and S2K_PK_AFFINE are the fast path. */
S2K_API int secp256k1_ec_pubkey_combine_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                              const unsigned char* keys, int key_format, const uint64_t* key_off, size_t n_sets);
S2K_API int secp256k1_ec_pubkey_combine_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                  const unsigned char* keys, int key_format, const uint64_t* key_off_host, size_t n_sets);

/* ---- SHA-256, tagged hashes and BIP-340 with a message length per item -------------------------------------------------
 * PUBLIC DATA ONLY.  The 32-byte digests that the verifiers of this header take (msghash32, msgs32, data32, the 32-byte messages
 * of BIP-340) are in practice SHA-256, double SHA-256 or tagged hashes of preimages of a few hundred bytes: these calls make them
 * on the GPU, one message per lane, so that a _dev verifier reads them where they were written.
 *   s2k_sha256_batch:              out32_i = SHA256(m_i) (rounds 1) or SHA256(SHA256(m_i)) (rounds 2); any other rounds is
 *                                  S2K_STATUS_ILLEGAL_ARGUMENT
 *   secp256k1_tagged_sha256_batch: out32_i = SHA256(SHA256(tag) | SHA256(tag) | m_i), byte for byte what
 *                                  secp256k1_tagged_sha256(ctx, out32_i, tag, taglen, m_i, len_i) writes (src/secp256k1.c:869-881).
 *                                  tag is HOST memory in both forms: its midstate is computed on the host and passed by value.
 * out32 is n*32 bytes.  The items:
 *   msg_off == NULL   item i is msgs[i*msglen .. (i+1)*msglen); msglen 0 is legal.
 *   msg_off != NULL   uint64_t[n+1]; item i is msgs[msg_off[i] .. msg_off[i+1]) and msglen is ignored (the sig_off convention of the
 *                     DER forms).  msg_off[0] need not be 0.
 * Only bytes inside an item are read: a buffer may end with its last item.
 * The host forms refuse offsets that decrease (S2K_STATUS_ILLEGAL_ARGUMENT, nothing written) and upload only the bytes
 * [msg_off[0], msg_off[n]).  The _dev forms take msgs, msg_off and out32 in HBM and cannot look at the offsets: an item with
 * msg_off[i+1] < msg_off[i] gets 32 zero bytes -- never the digest of the empty message -- and none of its bytes is read; its
 * neighbours are not affected.  n == 0 returns 1 and touches nothing; a NULL out32, tag or msgs is S2K_STATUS_ILLEGAL_ARGUMENT.
 * A wavefront runs as long as its longest message: sort by length first where lengths differ by orders of magnitude. */
S2K_API int s2k_sha256_batch(s2k_engine* e, unsigned char* out32, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, int rounds, size_t n);
S2K_API int s2k_sha256_batch_dev(s2k_engine* e, void* stream, unsigned char* out32, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, int rounds,
                                 size_t n);
S2K_API int secp256k1_tagged_sha256_batch(s2k_engine* e, unsigned char* out32, const unsigned char* tag, size_t taglen, const unsigned char* msgs,
                                          const uint64_t* msg_off, size_t msglen, size_t n);
S2K_API int secp256k1_tagged_sha256_batch_dev(s2k_engine* e, void* stream, unsigned char* out32, const unsigned char* tag, size_t taglen, const unsigned char* msgs,
                                              const uint64_t* msg_off, size_t msglen, size_t n);
/* secp256k1_tagged_sha256 with the reference's argument list (include/secp256k1.h), one item on the default engine; ctx is ignored.
 * Returns 1; 0 with S2K_STATUS_ILLEGAL_ARGUMENT for a NULL hash32, tag or msg (the reference's ARG_CHECKs, msglen 0 included). */
S2K_API int secp256k1_tagged_sha256_amd(const void* ctx, unsigned char* hash32, const unsigned char* tag, size_t taglen, const unsigned char* msg, size_t msglen);
/* results[i] = secp256k1_schnorrsig_verify(ctx, sig64_i, msg_i, msg_off[i+1] - msg_off[i], pubkey_i): secp256k1_schnorrsig_verify_batch
 * with a message length per item.  msgs and msg_off as above, msg_off required; sigs, pubkeys and pk_format as in
 * secp256k1_schnorrsig_verify_batch.  A decreasing pair of offsets: the host form refuses the call, the _dev form gives that item 0. */
S2K_API int secp256k1_schnorrsig_verify_batch_var(s2k_engine* e, int32_t* results, const unsigned char* sigs, const unsigned char* msgs, const uint64_t* msg_off,
                                                  const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_schnorrsig_verify_batch_var_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const unsigned char* msgs,
                                                      const uint64_t* msg_off, const unsigned char* pubkeys, int pk_format, size_t n);

/* ---- asset generators ----------------------------------------------------------------------------------------------
 * PUBLIC INPUTS ONLY: nothing below is constant time.  A blind handed to these functions is treated as public data (the
 * reference's generate_blinded and pedersen_commit are secret-key paths; here they serve explicit amounts, blind 0, and the
 * re-derivation of public objects).
 *
 * results[i] = secp256k1_generator_generate(ctx, &gens_out64[64 i], key32_i)                          (blinds32 NULL)
 *            = secp256k1_generator_generate_blinded(ctx, &gens_out64[64 i], key32_i, blind32_i)       (blinds32 n*32)
 *                                       (include/secp256k1_generator.h, src/modules/generator/main_impl.h:204-264; the map
 *                                        shallue_van_de_woestijne :94-202)
 * gens_out64 n*64: `secp256k1_generator` opaque objects, byte for byte the reference's.  Where results[i] == 0 -- a blind >= n --
 * the object is 64 zero bytes: the reference writes a generator from the reduced blind and returns 0, the engine does not.
 * (A key whose two mapped points are opposite, which no hash reaches and where the reference is undefined, gives 0 and zeros too.
 * So does a key one of whose two hashes is >= p, about 2^-128 per key: the reference returns 0 there as well but still writes a
 * generator.) */
S2K_API int secp256k1_generator_generate_batch(s2k_engine* e, int32_t* results, unsigned char* gens_out64, const unsigned char* keys32,
                                               const unsigned char* blinds32, size_t n);
S2K_API int secp256k1_generator_generate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* gens_out64, const unsigned char* keys32,
                                                   const unsigned char* blinds32, size_t n);
/* results[i] = secp256k1_generator_parse(ctx, &gens_out64[64 i], &gens33[33 i])            (src/modules/generator/main_impl.h:59-77)
 * gens33 n*33: prefix 0x0a / 0x0b, then x.  Any other prefix, x >= p or x off the curve gives 0 and 64 zero bytes.
 * out33[33 i ..] = what secp256k1_generator_serialize(ctx, out, &gens64[64 i]) writes: 11 ^ is_square(y), then x    (:79-92)
 * NULL where the reference has ARG_CHECK is S2K_STATUS_ILLEGAL_ARGUMENT (return 0); n == 0 returns 1.
 * _dev: every array in HBM; results and the outputs are zeroed on the stream first. */
S2K_API int secp256k1_generator_parse_batch(s2k_engine* e, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n);
S2K_API int secp256k1_generator_parse_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n);
S2K_API int secp256k1_generator_serialize_batch(s2k_engine* e, unsigned char* out33, const unsigned char* gens64, size_t n);
S2K_API int secp256k1_generator_serialize_batch_dev(s2k_engine* e, void* stream, unsigned char* out33, const unsigned char* gens64, size_t n);
/* ---- Pedersen commitments to public amounts -----------------------------------------------------------------------------
 * results[i] = secp256k1_pedersen_commit(ctx, &commit, blind32_i, values[i], &gens64[64 i])
 *                                       (src/modules/generator/main_impl.h:309-335, src/modules/generator/pedersen_impl.h:42-49)
 * commits_out33 n*33: the first 33 bytes of the commitment object (its serialisation): 9 ^ is_square(y), then x -- what
 * secp256k1_pedersen_verify_tally_batch takes.  blinds32 NULL: all-zero blinds, the explicit-amount case
 * (secp256k1_pedersen_commit(ctx, &c, zero_blind, value, &gen)); no fixed-base work is done then.
 * results[i] == 0 with 33 zero bytes: blind >= n, or the point at infinity (blind 0 with value 0; blind G = -value gen).
 * Generator objects are read as they are: one that is not on the curve is the caller's error, as in the reference, and the error
 * stays with its item.  The all-zero object -- what the parse and generate forms above write for a refused item -- and any other
 * object with y = 0 are refused: results[i] == 0 and 33 zero bytes, whatever value and blind are.  Other off-curve objects give
 * some 33 bytes, or 0 and zero bytes.  The other items of the batch are never affected. */
S2K_API int secp256k1_pedersen_commit_batch(s2k_engine* e, int32_t* results, unsigned char* commits_out33, const unsigned char* blinds32,
                                            const uint64_t* values, const unsigned char* gens64, size_t n);
S2K_API int secp256k1_pedersen_commit_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* commits_out33, const unsigned char* blinds32,
                                                const uint64_t* values, const unsigned char* gens64, size_t n);

/* ---- half-aggregated Schnorr signature verification ------------------------------------------------------------------
 * *result = secp256k1_schnorrsig_aggverify(ctx, pubkeys, msgs32, n, aggsig, aggsig_len)
 *                                       (include/secp256k1_schnorrsig_halfagg.h, src/modules/schnorrsig_halfagg/main_impl.h:108-198)
 * evaluated as one (2n+1)-term multi-scalar multiplication  -s*G + sum z_i*R_i + sum (z_i e_i)*P_i == infinity  on the GPU
 * (the reference does two single multiplications per signature).  pubkeys / pk_format as in the BIP-340 batch call
 * (0 = n*32 serialised x-only keys, 1 = n*64 secp256k1_xonly_pubkey objects); msgs32 n*32; aggsig = r_0|...|r_{n-1}|s,
 * aggsig_len must be 32*(n+1) or the verdict is 0.  The return value is the call's success, the verdict goes to *result. */
S2K_API int secp256k1_schnorrsig_aggverify_amd(s2k_engine* e, int32_t* result, const unsigned char* pubkeys, int pk_format,
                                               const unsigned char* msgs32, size_t n, const unsigned char* aggsig, size_t aggsig_len);

/* ---- half-aggregated Schnorr signatures: many aggregates per call, verification and aggregation ---------------------------
 * One aggregate per call is a chain of latency-bound launches behind a serial hash chain; a caller with one small aggregate per
 * transaction or per block has thousands of them.  These calls take K aggregates at once: one hash chain per GPU lane, the per-signature
 * work one lane per signature over the whole batch, and the K sums in one launch chain (as s2k_ecmult_multi_many).  With both sides a
 * node goes from signatures to aggregates to verdicts without leaving HBM.  All public data; nothing here is constant time.
 * Conventions as in the MuSig2 aggregation section: results[] per aggregate; 0 and zeroed outputs for a refused aggregate, neighbours
 * never affected; S2K_STATUS_ILLEGAL_ARGUMENT only for NULL where the reference has ARG_CHECK, a pk_format out of range, offsets that
 * do not start at 0 or that decrease, n_before[k] above the aggregate's item count, and a batch above what one call indexes (2^40
 * signatures, 2^46 aggregate bytes or 2^31 aggregates: "batch too large").  In the _dev forms every byte array is in HBM,
 * results and outputs are zeroed on the stream first, and item_off, aggsig_off and n_before are HOST arrays (n_aggs + 1, n_aggs + 1
 * and n_aggs entries), read before the call returns.  n_aggs == 0 returns 1.
 * item_off counts signatures: aggregate k owns keys and messages [item_off[k], item_off[k+1]) of the back-to-back arrays (n_k of them).
 * pk_format as above: 0 = 32-byte serialised x-only keys, 1 = 64-byte secp256k1_xonly_pubkey objects.
 *
 * results[k] = secp256k1_schnorrsig_aggverify(ctx, keys_k, msgs_k, n_k, aggsigs + aggsig_off[k], aggsig_off[k+1] - aggsig_off[k])
 *                                       (src/modules/schnorrsig_halfagg/main_impl.h:108-198)
 * aggsig_off holds BYTE offsets into aggsigs (like proof_off).  An aggregate whose length is not 32 (n_k + 1) gets verdict 0 and
 * costs no key work (:122-125).  n_k == 0 is legal: the verdict is 1 exactly when s == 0.  An aggregate of more than 4 096
 * signatures goes through the single-aggregate path (secp256k1_schnorrsig_aggverify_dev) behind the others, inside the same call.
 *
 * results[k] = secp256k1_schnorrsig_aggregate(ctx, out_k, &len, keys_k, msgs_k, sigs_k, n_k)              (:104-106, :19-102)
 * sigs64: the n_k BIP-340 signatures of every aggregate, back to back (64 bytes each, item order).  Aggregate k is written at byte
 * 32 (item_off[k] + k) of aggsigs_out and is 32 (n_k + 1) bytes long, so the output feeds the verifier with
 * aggsig_off[k] = 32 (item_off[k] + k); aggsigs_out needs 32 (item_off[n_aggs] + n_aggs) bytes.  As in the reference s_i is reduced,
 * not refused, and r_i is not checked.  results[k] == 0: a format-0 key that secp256k1_xonly_pubkey_parse refuses, or an all-zero
 * key object (where the reference's xonly_pubkey_serialize fails).  DIFFERENCE FROM THE REFERENCE: the aggregate's 32 (n_k + 1)
 * output bytes are then zero; the reference leaves the buffer untouched.
 *
 * results[k] = secp256k1_schnorrsig_inc_aggregate(ctx, out_k (holding aggregate k of aggsigs_in), &len, keys_k, msgs_k, new sigs of k,
 *                                                 n_before[k], n_k - n_before[k])                          (:19-102)
 * aggsigs_in: aggregate k is 32 (n_before[k] + 1) bytes (r_0 .. r_{n_before-1} | s_old), the aggregates packed back to back.
 * new_sigs64: the n_k - n_before[k] new signatures of every aggregate, back to back.  The output layout is the aggregation call's
 * (the old r_i are copied over).  As in the reference s_old is read without an overflow check, and only when n_before[k] > 0.
 * secp256k1_schnorrsig_aggregate_batch is this call with every count 0 (and no aggsigs_in).
 *
 * Sizes.  The hash chain of ONE aggregate is walked by one GPU lane, about 3 us per 64-byte block and 1.5 blocks per signature, in the
 * verifier up to 4 096 signatures per aggregate and in the aggregation calls whatever n_k is: these calls are for MANY aggregates of up
 * to a few thousand signatures.  An aggregate of 2^20 signatures keeps a single kernel busy for about 5 s and the host plan takes 8
 * bytes per signature of the longest aggregate; aggregate such a set in pieces (the incremental call continues an aggregate) or with
 * the reference.
 * Timing.  s2k_engine_last_ms(0) spans the call's launches, except that after a verification batch holding an over-limit aggregate it
 * spans only the last single-aggregate launch; s2k_engine_last_ms(1) is the chain kernel in the aggregation calls and the bucket sums
 * of the many-sums chain in the verification call (take the chain's time from an aggregation call over the same bytes).
 *
 * Out of scope: group forms of these calls, the hook into the reference's own functions (integration/), and bench.py. */
S2K_API int secp256k1_schnorrsig_aggverify_batch(s2k_engine* e, int32_t* results, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                 const uint64_t* item_off, const unsigned char* aggsigs, const uint64_t* aggsig_off, size_t n_aggs);
S2K_API int secp256k1_schnorrsig_aggverify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* pubkeys, int pk_format,
                                                     const unsigned char* msgs32, const uint64_t* item_off, const unsigned char* aggsigs,
                                                     const uint64_t* aggsig_off, size_t n_aggs);
S2K_API int secp256k1_schnorrsig_aggregate_batch(s2k_engine* e, int32_t* results, unsigned char* aggsigs_out, const unsigned char* pubkeys, int pk_format,
                                                 const unsigned char* msgs32, const unsigned char* sigs64, const uint64_t* item_off, size_t n_aggs);
S2K_API int secp256k1_schnorrsig_aggregate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggsigs_out, const unsigned char* pubkeys,
                                                     int pk_format, const unsigned char* msgs32, const unsigned char* sigs64, const uint64_t* item_off,
                                                     size_t n_aggs);
S2K_API int secp256k1_schnorrsig_inc_aggregate_batch(s2k_engine* e, int32_t* results, unsigned char* aggsigs_out, const unsigned char* aggsigs_in,
                                                     const uint64_t* n_before, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                     const unsigned char* new_sigs64, const uint64_t* item_off, size_t n_aggs);
S2K_API int secp256k1_schnorrsig_inc_aggregate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggsigs_out, const unsigned char* aggsigs_in,
                                                         const uint64_t* n_before, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                         const unsigned char* new_sigs64, const uint64_t* item_off, size_t n_aggs);

/* ---- BIP-340: one verdict for a whole batch, as a single multi-scalar multiplication ------------------------------------------
 * *verdict = AND over i of secp256k1_schnorrsig_verify(ctx, sig64_i, msg_i, msglen, pubkey_i)
 *                                       (include/secp256k1_schnorrsig.h, src/modules/schnorrsig/main_impl.h:215-261; challenge :106-120)
 * The reference has no batch verifier; this is the one BIP-340 describes.  For a block validator or an indexer that only needs to know
 * whether ALL signatures are valid:  -(sum a_i s_i) G + sum a_i R_i + sum (a_i e_i) P_i == infinity,  R_i = lift_x(r_i), one
 * (2n+1)-term sum (points R_0, P_0, R_1, P_1, ... as in the half-aggregate verifier) instead of n double multiplications.
 * The verdict is 0 whenever some r_i >= p, r_i is not an x coordinate, s_i >= n or a key does not parse (an all-zero key object
 * included) -- the refusals of :231-242, and an r_i that no R can match (:260) -- and otherwise 1 exactly when the equation holds.  A batch of valid signatures is never
 * refused; a batch holding an invalid one is accepted with probability at most 2^-128 over the hash that gives the coefficients.
 *
 * The coefficients a_i come from the batch itself through a hash TREE (16 children per node, one GPU lane per node, one launch per
 * level), so that every a_i depends on every byte of the batch and nothing is serial beyond the tree's depth:
 *   T(tag, x) = SHA256(SHA256(tag) | SHA256(tag) | x)
 *   d_i  = T("S2K/schnorr_all/item", sig_i | x32_i | m_i)      x32_i: the key's 32 serialised bytes (pk_format 1: the object's x, big-endian)
 *   node j of the next level = T("S2K/schnorr_all/node", nodes 16j .. min(16j+16, count)-1 of this level), from d_0 .. d_{n-1} until one is left
 *   seed = T("S2K/schnorr_all/seed", le64(n) | le64(msglen) | root)                                (n = 1: root = d_0)
 *   a_0 = 1;  a_i = the first 16 bytes, big-endian, of T("S2K/schnorr_all/rand", seed | le64(i)), 0 replaced by 1
 * seed32_out (or NULL) receives the seed: it pins the derivation for tests and lets two parties compare what they verified.
 *
 * sigs n*64, msgs n*msglen (msglen uniform, may be 0), pubkeys / pk_format as in secp256k1_schnorrsig_verify_batch (0 = n*32
 * serialised x-only keys, 1 = n*64 secp256k1_xonly_pubkey objects).  The return value is the call's success, the verdict goes to
 * *verdict.  NULL where the reference has ARG_CHECK, or a pk_format out of range, is S2K_STATUS_ILLEGAL_ARGUMENT (return 0), and so
 * is a batch of more terms than one sum indexes (2n + 1 above 238 609 293, or S2K_OPT_MSM_MAX_TERMS: "batch too large").
 * n == 0 returns 1 with verdict 1 and 32 zero bytes as the seed.
 * results (n entries, or NULL), host form only: when the verdict is 0 the per-item verifier (secp256k1_schnorrsig_verify_batch_dev)
 * runs on the buffers already uploaded and results[] says which items failed; when it is 1 results[] is all ones.
 * The _dev form: every array in HBM, stream-ordered, never synchronises and writes only verdict_dev[0] and, if asked for, the 32
 * seed bytes; a caller that wants locations calls secp256k1_schnorrsig_verify_batch_dev itself.
 * Timing.  s2k_engine_last_ms(0) spans the call's launches (after a locating host call: the per-item verifier's), s2k_engine_last_ms(1)
 * is the multi-scalar multiplication.  s2k_schnorr_all_last_split_ms: the phases of the most recent call of the engine, in ms, valid
 * once its work is complete -- out4[0] lift, item digests and challenges, [1] hash tree and seed, [2] coefficients, scalar products
 * and the sum of a_i s_i, [3] the multi-scalar multiplication; -1 where there is nothing to report.
 *
 * Out of scope: group forms, the hook into the reference's own functions (integration/), bench.py, several batches per call,
 * Taproot tweak checks inside the batch, caller-supplied randomness, and automatic dispatch between this call and the per-item one. */
S2K_API int secp256k1_schnorrsig_verify_all(s2k_engine* e, int32_t* verdict, int32_t* results, unsigned char* seed32_out, const unsigned char* sigs,
                                            const unsigned char* msgs, size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_schnorrsig_verify_all_dev(s2k_engine* e, void* stream, int32_t* verdict_dev, unsigned char* seed32_out_dev, const unsigned char* sigs,
                                                const unsigned char* msgs, size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int s2k_schnorr_all_last_split_ms(s2k_engine* e, float* out4);

/* ---- Borromean rangeproof batch verification ---------------------------------------------------------------------
 * results[i], min_value[i], max_value[i] = secp256k1_rangeproof_verify(ctx, &min, &max, commit_i, proof_i, plen_i,
 *                                          extra_commit_i, extra_commit_len_i, gen_i)
 *                                       (include/secp256k1_rangeproof.h:70-80, src/modules/rangeproof/main_impl.h:54-71,
 *                                        rangeproof_impl.h:541-683, borromean_impl.h:53-104)
 * Packed form: proofs = all proofs back to back, proof_off[n+1] byte offsets (proof i = [off[i], off[i+1]));
 * commits n*33 = serialised Pedersen commitments (equivalently the first 33 bytes of each 64-byte
 * secp256k1_pedersen_commitment object; an encoding that secp256k1_pedersen_commitment_parse refuses -- a prefix other than 8 / 9, x >= p,
 * x not on the curve -- can never be such an object and gives results[i] = 0); gens n*64 = secp256k1_generator objects; extra / extra_off
 * likewise or NULL.
 * min_value / max_value are written exactly when the reference writes them (header parsed), starting from 0. */
S2K_API int secp256k1_rangeproof_verify_batch(s2k_engine* e, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                              const unsigned char* commits33, const unsigned char* proofs, const uint64_t* proof_off,
                                              const unsigned char* extra, const uint64_t* extra_off, const unsigned char* gens64, size_t n);
/* The same batch given the way the reference's own callers hold it -- arrays of pointers to the objects: commit_objs[i] -> a
 * secp256k1_pedersen_commitment (its first 33 bytes are read: src/modules/generator/main_impl.h:266-279), proofs[i] / plens[i],
 * extra[i] / elens[i] (extra may be NULL; extra[i] may be NULL when elens[i] == 0), gen_objs[i] -> a secp256k1_generator (64 bytes).
 * Both host-buffer forms gather their inputs once, with a few host threads ($S2K_STAGE_THREADS, default min(8, cores / 2)), straight into
 * pinned staging memory and copy it to HBM piece by piece underneath the packing; results come back through pinned memory. */
S2K_API int secp256k1_rangeproof_verify_batch_ptrs(s2k_engine* e, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                   const void* const* commit_objs, const unsigned char* const* proofs, const size_t* plens,
                                                   const unsigned char* const* extra, const size_t* elens, const void* const* gen_objs, size_t n);
/* Asynchronous pair over the two host-buffer forms, for callers with a stream of batches (the blocks of a chain sync, the transactions of a
 * mempool): `_submit` gathers the inputs, queues the copies and the kernels and returns a ticket; `_wait(ticket)` blocks until that batch is
 * done and only then fills results / min_value / max_value (which must stay valid until then; `results` holds zeros in between).  The
 * INPUT arrays may be reused as soon as `_submit` returns.  At most TWO submissions may be in flight -- a third `_submit` fails
 * (S2K_STATUS_BUSY) until the older ticket has been waited for -- and tickets may be waited for in any order, from any thread.  With
 *     submit(k+1); wait(k); submit(k+2); wait(k+1); ...
 * the gathering and the PCIe copies of batch k+1 run underneath the kernels of batch k and the GPU never idles: the throughput of the
 * host-buffer path becomes that of the device-resident one (bench.py: dropin.two_in_flight).  The synchronous forms above are
 * submit + wait on one of the same two staging sets: concurrent synchronous callers (verifier threads sharing an engine) queue for a
 * set -- two of them overlap, none is turned away -- unless both sets are held by asynchronous tickets, which only the application can
 * free: the synchronous call then returns 0 at once with S2K_STATUS_BUSY.
 * A ticket is never 0. */
S2K_API int secp256k1_rangeproof_verify_batch_submit(s2k_engine* e, uint64_t* ticket, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                     const unsigned char* commits33, const unsigned char* proofs, const uint64_t* proof_off,
                                                     const unsigned char* extra, const uint64_t* extra_off, const unsigned char* gens64, size_t n);
S2K_API int secp256k1_rangeproof_verify_batch_ptrs_submit(s2k_engine* e, uint64_t* ticket, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                          const void* const* commit_objs, const unsigned char* const* proofs, const size_t* plens,
                                                          const unsigned char* const* extra, const size_t* elens, const void* const* gen_objs, size_t n);
S2K_API int secp256k1_rangeproof_verify_batch_wait(s2k_engine* e, uint64_t ticket);
S2K_API int secp256k1_rangeproof_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                  const unsigned char* commits33, const unsigned char* proofs, const uint64_t* proof_off,
                                                  const unsigned char* extra, const uint64_t* extra_off, const unsigned char* gens64, size_t n);
/* Rewind: verification as above and, for the proofs that verify, recovery of the committed value, the blinding factor and the
 * embedded message from the nonce -- per item what
 *   secp256k1_rangeproof_rewind(ctx, blind_out, &value_out, message_out, &outlen, nonce, &min, &max, commit, proof, plen,
 *                               extra_commit, extra_commit_len, gen)   (include/secp256k1_rangeproof.h:102-130,
 *                               src/modules/rangeproof/main_impl.h:31-52, rangeproof_impl.h:61-108,339-485,652-680)
 * returns and writes.  nonces n*32; blind_out n*32; value_out n; message_out n*msg_stride or NULL; outlen n (in: capacity of
 * item i's message buffer, at most msg_stride; out: bytes recovered) -- required iff message_out is given.  Items with
 * results[i] == 0 get zeroed blind/value and outlen 0.  Nonces are secrets: they are copied to the GPU. */
S2K_API int secp256k1_rangeproof_rewind_batch(s2k_engine* e, int32_t* results, unsigned char* blind_out, uint64_t* value_out, unsigned char* message_out,
                                              uint64_t* outlen, size_t msg_stride, const unsigned char* nonces, uint64_t* min_value, uint64_t* max_value,
                                              const unsigned char* commits33, const unsigned char* proofs, const uint64_t* proof_off,
                                              const unsigned char* extra, const uint64_t* extra_off, const unsigned char* gens64, size_t n);
/* Single-item form with the reference's argument list (ctx is accepted and ignored: the engine is process-global,
 * lazily created on device $S2K_DEVICE or 0).  commit / gen point at the reference's 64-byte opaque objects. */
S2K_API int secp256k1_rangeproof_verify_amd(const void* ctx, uint64_t* min_value, uint64_t* max_value, const void* commit,
                                            const unsigned char* proof, size_t plen, const unsigned char* extra_commit,
                                            size_t extra_commit_len, const void* gen);

/* Further single-item forms with the reference's argument lists (ctx ignored; same process-global engine; see
 * s2k_last_status() for telling "invalid" from "engine failed"):
 *   secp256k1_schnorrsig_verify(ctx, sig64, msg, msglen, pubkey)                       include/secp256k1_schnorrsig.h:178
 *   secp256k1_pedersen_verify_tally(ctx, commits, pcnt, ncommits, ncnt)                include/secp256k1_generator.h:190
 *   secp256k1_surjectionproof_verify(ctx, proof, input_tags, n_input_tags, output_tag) include/secp256k1_surjectionproof.h:256
 * Pointers to opaque objects are passed as const void* (64-byte xonly_pubkey / pedersen_commitment / generator objects,
 * the secp256k1_surjectionproof struct). */
S2K_API int secp256k1_schnorrsig_verify_amd(const void* ctx, const unsigned char* sig64, const unsigned char* msg, size_t msglen, const void* pubkey);
S2K_API int secp256k1_pedersen_verify_tally_amd(const void* ctx, const void* const* commits, size_t pcnt, const void* const* ncommits, size_t ncnt);
S2K_API int secp256k1_surjectionproof_verify_amd(const void* ctx, const void* proof, const void* ephemeral_input_tags, size_t n_ephemeral_input_tags,
                                                 const void* ephemeral_output_tag);
/*   secp256k1_ecdsa_verify(ctx, sig, msghash32, pubkey)                                include/secp256k1.h:622
 *   secp256k1_ecdsa_recover(ctx, pubkey, sig, msghash32)                               include/secp256k1_recovery.h:112
 * sig: the 64-byte secp256k1_ecdsa_signature object / the 65-byte secp256k1_ecdsa_recoverable_signature object (the limbs of
 * r and s, then the recovery id); pubkey: the 64-byte secp256k1_pubkey object (written by the recovery form: zeroed on failure). */
S2K_API int secp256k1_ecdsa_verify_amd(const void* ctx, const void* sig, const unsigned char* msghash32, const void* pubkey);
S2K_API int secp256k1_ecdsa_recover_amd(const void* ctx, void* pubkey, const void* signature, const unsigned char* msghash32);
/*   secp256k1_ecdsa_adaptor_verify(ctx, adaptor_sig162, pubkey, msg32, enckey)         include/secp256k1_ecdsa_adaptor.h,
 *                                                                                      src/modules/ecdsa_adaptor/main_impl.h:236
 * pubkey, enckey: 64-byte secp256k1_pubkey objects. */
S2K_API int secp256k1_ecdsa_adaptor_verify_amd(const void* ctx, const unsigned char* adaptor_sig162, const void* pubkey, const unsigned char* msg32,
                                               const void* enckey);
/*   secp256k1_ecdsa_s2c_verify_commit(ctx, sig, data32, opening)                       include/secp256k1_ecdsa_s2c.h,
 *                                                                                      src/modules/ecdsa_s2c/main_impl.h:88
 *   secp256k1_anti_exfil_host_verify(ctx, sig, msg32, pubkey, host_data32, opening)    src/modules/ecdsa_s2c/main_impl.h:185
 * sig: the 64-byte secp256k1_ecdsa_signature object; pubkey, opening: 64-byte secp256k1_pubkey / secp256k1_ecdsa_s2c_opening objects. */
S2K_API int secp256k1_ecdsa_s2c_verify_commit_amd(const void* ctx, const void* sig, const unsigned char* data32, const void* opening);
S2K_API int secp256k1_anti_exfil_host_verify_amd(const void* ctx, const void* sig, const unsigned char* msg32, const void* pubkey, const unsigned char* host_data32,
                                                 const void* opening);
/*   secp256k1_ellswift_decode(ctx, pubkey, ell64)                                      include/secp256k1_ellswift.h,
 *                                                                                      src/modules/ellswift/main_impl.h:470
 *   secp256k1_ellswift_encode(ctx, ell64, pubkey, rnd32)                               src/modules/ellswift/main_impl.h:393
 * pubkey: the 64-byte secp256k1_pubkey object.  decode returns 1 (0 + S2K_STATUS_ENGINE_FAILURE and a zeroed object when the engine failed). */
S2K_API int secp256k1_ellswift_decode_amd(const void* ctx, void* pubkey, const unsigned char* ell64);
S2K_API int secp256k1_ellswift_encode_amd(const void* ctx, unsigned char* ell64, const void* pubkey, const unsigned char* rnd32);
/*   secp256k1_musig_partial_sig_verify(ctx, partial_sig, pubnonce, pubkey, keyagg_cache, session)      include/secp256k1_musig.h,
 *                                                                                      src/modules/musig/session_impl.h:716
 * all five point at the reference's objects (36, 132, 64, 197 and 133 bytes). */
S2K_API int secp256k1_musig_partial_sig_verify_amd(const void* ctx, const void* partial_sig, const void* pubnonce, const void* pubkey, const void* keyagg_cache,
                                                   const void* session);
/*   secp256k1_musig_pubkey_agg(ctx, agg_pk, keyagg_cache, pubkeys, n_pubkeys)          include/secp256k1_musig.h,
 *                                                                                      src/modules/musig/keyagg_impl.h:156
 * pubkeys: n_pubkeys pointers to 64-byte secp256k1_pubkey objects; agg_pk (64 bytes) and keyagg_cache (197 bytes) may each be NULL. */
S2K_API int secp256k1_musig_pubkey_agg_amd(const void* ctx, void* agg_pk, void* keyagg_cache, const void* const* pubkeys, size_t n_pubkeys);
/*   secp256k1_whitelist_verify(ctx, sig, online_pubkeys, offline_pubkeys, n_keys, sub_pubkey)      include/secp256k1_whitelist.h
 * sig: the secp256k1_whitelist_signature object {size_t n_keys; unsigned char data[32 * 256]}; the key arrays: n_keys 64-byte
 * secp256k1_pubkey objects each (they may be NULL when n_keys is 0 here; the reference's ARG_CHECK refuses that). */
S2K_API int secp256k1_whitelist_verify_amd(const void* ctx, const void* sig, const void* online_pubkeys, const void* offline_pubkeys, size_t n_keys,
                                           const void* sub_pubkey);
/*   secp256k1_xonly_pubkey_tweak_add_check(ctx, tweaked_pubkey32, tweaked_pk_parity, internal_pubkey, tweak32)
 *                                                                   include/secp256k1_extrakeys.h, src/modules/extrakeys/main_impl.h:135
 *   secp256k1_xonly_pubkey_tweak_add(ctx, output_pubkey, internal_pubkey, tweak32)          src/modules/extrakeys/main_impl.h:118
 *   secp256k1_ec_pubkey_tweak_add(ctx, pubkey, tweak32)                                     src/secp256k1.c:773
 * internal_pubkey: the 64-byte secp256k1_xonly_pubkey object; output_pubkey / pubkey: 64-byte secp256k1_pubkey objects (pubkey
 * is read and written; both are zeroed on failure as the reference does).  A parity other than 0 or 1 gives 0 without a launch. */
S2K_API int secp256k1_xonly_pubkey_tweak_add_check_amd(const void* ctx, const unsigned char* tweaked_pubkey32, int tweaked_pk_parity,
                                                       const void* internal_pubkey, const unsigned char* tweak32);
S2K_API int secp256k1_xonly_pubkey_tweak_add_amd(const void* ctx, void* output_pubkey, const void* internal_pubkey, const unsigned char* tweak32);
S2K_API int secp256k1_ec_pubkey_tweak_add_amd(const void* ctx, void* pubkey, const unsigned char* tweak32);
/*   secp256k1_ec_pubkey_parse(ctx, pubkey, input, inputlen)                          src/secp256k1.c:290
 *   secp256k1_ec_pubkey_serialize(ctx, output, outputlen, pubkey, flags)             src/secp256k1.c:308
 *   secp256k1_ec_pubkey_negate(ctx, pubkey)                                          src/secp256k1.c:723
 *   secp256k1_ec_pubkey_tweak_mul(ctx, pubkey, tweak32)                              src/secp256k1.c:810
 *   secp256k1_ec_pubkey_combine(ctx, out, ins, n)                                    src/secp256k1.c:843
 *   secp256k1_xonly_pubkey_parse(ctx, pubkey, input32)                               src/modules/extrakeys/main_impl.h:22
 *   secp256k1_xonly_pubkey_serialize(ctx, output32, pubkey)                          src/modules/extrakeys/main_impl.h:44
 *   secp256k1_xonly_pubkey_from_pubkey(ctx, xonly_pubkey, pk_parity, pubkey)         src/modules/extrakeys/main_impl.h:85
 * pubkey / xonly_pubkey / out: 64-byte objects, zeroed first wherever the reference does; an inputlen other than 33 or 65 gives 0
 * without a launch; flags: SECP256K1_EC_COMPRESSED (258) or SECP256K1_EC_UNCOMPRESSED (2), *outputlen in: the buffer's size, out:
 * 33 / 65 (0 on failure); ins: n pointers to objects; pk_parity may be NULL. */
S2K_API int secp256k1_ec_pubkey_parse_amd(const void* ctx, void* pubkey, const unsigned char* input, size_t inputlen);
S2K_API int secp256k1_ec_pubkey_serialize_amd(const void* ctx, unsigned char* output, size_t* outputlen, const void* pubkey, unsigned int flags);
S2K_API int secp256k1_ec_pubkey_negate_amd(const void* ctx, void* pubkey);
S2K_API int secp256k1_ec_pubkey_tweak_mul_amd(const void* ctx, void* pubkey, const unsigned char* tweak32);
S2K_API int secp256k1_ec_pubkey_combine_amd(const void* ctx, void* out, const void* const* ins, size_t n);
S2K_API int secp256k1_xonly_pubkey_parse_amd(const void* ctx, void* pubkey, const unsigned char* input32);
S2K_API int secp256k1_xonly_pubkey_serialize_amd(const void* ctx, unsigned char* output32, const void* pubkey);
S2K_API int secp256k1_xonly_pubkey_from_pubkey_amd(const void* ctx, void* xonly_pubkey, int* pk_parity, const void* pubkey);
/*   secp256k1_generator_generate(ctx, gen, key32)                                  src/modules/generator/main_impl.h:250
 *   secp256k1_generator_parse(ctx, gen, input)                                     src/modules/generator/main_impl.h:59
 *   secp256k1_pedersen_commit(ctx, commit, blind, value, gen)                      src/modules/generator/main_impl.h:309
 * gen: the 64-byte secp256k1_generator object; commit: the 64-byte secp256k1_pedersen_commitment object, of which the first 33
 * bytes are written and the rest zeroed.  Outputs are zeroed on failure.  The blind is treated as public data (see above). */
S2K_API int secp256k1_generator_generate_amd(const void* ctx, void* gen, const unsigned char* key32);
S2K_API int secp256k1_generator_parse_amd(const void* ctx, void* gen, const unsigned char* input33);
S2K_API int secp256k1_pedersen_commit_amd(const void* ctx, void* commit, const unsigned char* blind, uint64_t value, const void* gen);

/* ---- Pedersen commitment tallies ------------------------------------------------------------------------------------
 * results[t] = secp256k1_pedersen_verify_tally(ctx, pos_t, pcnt_t, neg_t, ncnt_t)
 *                                       (include/secp256k1_generator.h:174-196, src/modules/generator/main_impl.h:371-396)
 * commits33: all commitments of all tallies back to back in serialised form (33 bytes; equivalently the first 33 bytes of each
 * secp256k1_pedersen_commitment object); tally t owns commitments [tally_off[t], tally_off[t+1]) and the first n_pos[t] of them
 * are its positive list, the rest its negative list.  A commitment that is not a valid encoding (cannot come out of
 * secp256k1_pedersen_commitment_parse) makes its tally 0. */
S2K_API int secp256k1_pedersen_verify_tally_batch(s2k_engine* e, int32_t* results, const unsigned char* commits33, const uint64_t* tally_off,
                                                  const uint64_t* n_pos, size_t n_tallies);

/* ---- surjection-proof batch verification -----------------------------------------------------------------------------
 * results[i] = secp256k1_surjectionproof_parse(ctx, &proof, ser_i, len_i) &&
 *              secp256k1_surjectionproof_verify(ctx, &proof, ephemeral_input_tags_i, n_i, &ephemeral_output_tag_i)
 *                                       (include/secp256k1_surjectionproof.h, src/modules/surjection/main_impl.h:45-82,360-402)
 * proofs: serialised proofs back to back with proof_off[n+1]; input_tags64: all items' input generators (64-byte
 * secp256k1_generator objects) back to back with tag_off[n+1] counted in tags; output_tags64: n*64. */
S2K_API int secp256k1_surjectionproof_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* proofs, const uint64_t* proof_off,
                                                   const unsigned char* input_tags64, const uint64_t* tag_off, const unsigned char* output_tags64, size_t n);
S2K_API int secp256k1_surjectionproof_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* proofs,
                                                       const uint64_t* proof_off, const unsigned char* input_tags64, const uint64_t* tag_off,
                                                       const unsigned char* output_tags64, size_t n);

/* ---- Bulletproofs++ norm-argument batch verification ---------------------------------------------------------------
 * results[i] = secp256k1_bppp_rangeproof_norm_product_verify(ctx, scratch, proof_i, proof_len, &transcript_i, &rho_i,
 *                                       g_vec, g_len, c_vec_i, c_vec_len, &commit_i)
 *                                       (src/modules/bppp/bppp_norm_product_impl.h:425-552)
 * All items share the generator set (gens33: n_gens compressed points, G_i first then H_i, as
 * secp256k1_bppp_generators_serialize writes them), g_len, c_vec_len and proof_len.  transcripts: n * 104 bytes, each the
 * SHA-256 state {uint32 s[8]; uint8 buf[64]; uint64 bytes} of the parent protocol (src/hash.h); rho n*32; c_vec
 * n*c_vec_len*32; commits n*33 (33 zero bytes = infinity, secp256k1.c:895).
 * The engine keeps a fixed-base table for the most recent generator set (75.5 MB per generator, built on the first call with that
 * set and reused while gens33 stays byte-identical); sets of more than 256 generators take the table-free path. */
S2K_API int secp256k1_bppp_norm_product_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* proofs, size_t proof_len,
                                                     const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33,
                                                     size_t n_gens, size_t g_len, const unsigned char* c_vec, size_t c_vec_len,
                                                     const unsigned char* commits33, size_t n);

/* ---- Bulletproofs++ norm arguments: one verdict for a whole batch over ONE generator set, as a single multi-scalar multiplication ----
 * *verdict = AND over p of secp256k1_bppp_rangeproof_norm_product_verify(ctx, scratch, proof_p, proof_len, &transcript_p, &rho_p,
 *                                       g_vec, g_len, c_vec_p, c_vec_len, &commit_p)      (src/modules/bppp/bppp_norm_product_impl.h:425-552)
 * The reference verifies one proof per call (a `static`); this is how Bulletproofs are verified in bulk.  With sc[p][t] the scalars the
 * per-item verifier multiplies proof p's terms by (generators, G, -1 for the commitment, -gamma_i and -(gamma_i^2 - 1) for X_i and R_i)
 * and D_p = sum_t sc[p][t] P_{p,t} the sum it requires to be infinity, the call checks  sum_p z'_p D_p == infinity  as ONE sum:
 *   generator t:  S_t = sum_p z'_p sc[p][t] mod n   (n_gens terms for the whole batch)       G:  sum_p z'_p v_p
 *   per proof:    the commitment with -z'_p, X_{p,i} with -z'_p gamma_{p,i}, R_{p,i} with -z'_p (gamma_{p,i}^2 - 1)     (2 n_rounds + 1 terms)
 * The verdict is 0 for a shape the reference refuses (:446-461); 0 whenever for ANY proof n or l overflows, rho is 0, or a generator,
 * the commitment or an X / R does not parse; otherwise 1 exactly when the sum is infinity.  A batch of valid proofs is never refused;
 * a batch holding an invalid one is accepted with probability at most 2^-128 over the hash that gives the coefficients:
 *   T(tag, x) = SHA256(SHA256(tag) | SHA256(tag) | x)
 *   gd   = T("S2K/bppp_all/gens", le64(n_gens) | le64(g_len) | gens33)
 *   d_p  = T("S2K/bppp_all/item", proof_p | transcript104_p | rho_p | c_vec_p | commit33_p)
 *   node j of the next level = T("S2K/bppp_all/node", nodes 16j .. min(16j+16, count)-1 of this level), from d_0 .. d_{n-1} until one is left
 *   seed = T("S2K/bppp_all/seed", le64(n) | le64(proof_len) | le64(c_vec_len) | gd | root)                   (n = 1: root = d_0)
 *   z_0 = 1;  z_p = the first 16 bytes, big-endian, of T("S2K/bppp_all/rand", seed | le64(p)), 0 replaced by 1
 *   z'_p = mu z_p mod n,  mu = SHA256("S2K/bppp_all/scale") mod n   (one public factor on every scalar: the statement is unchanged)
 * All 104 bytes of a transcript object are hashed as given: the bytes of its buffer beyond the fill level change the seed and never
 * the verdict.  seed32_out (or NULL) receives the seed.
 *
 * Arrays as in secp256k1_bppp_norm_product_verify_batch.  The return value is the call's success, the verdict goes to *verdict.  A NULL
 * array with n > 0 or a NULL verdict is S2K_STATUS_ILLEGAL_ARGUMENT (return 0), and so is a batch of more terms than one sum indexes
 * (n_gens + n (2 n_rounds + 1) above the limit of s2k_ecmult_multi, or S2K_OPT_MSM_MAX_TERMS: "batch too large"); g_len above 256 is
 * the engine-level failure of the per-item call.  n == 0 returns 1 with verdict 1 and 32 zero bytes as the seed; a refused shape
 * leaves 32 zero bytes as well.
 * results (n entries, or NULL), host form only: when the verdict is 0 the per-item verifier runs on the buffers already uploaded and
 * results[] says which proofs failed; when it is 1 results[] is all ones.
 * The _dev form: every array in HBM (gens33_host: the set once more on the host, hashed into gd there), stream-ordered, never
 * synchronises and writes only verdict_dev[0] and, if asked for, the 32 seed bytes.  It neither needs nor builds the set's fixed-base table.
 * s2k_bppp_all_last_split_ms: the phases of the engine's most recent call, in ms, valid once its work is complete -- out4[0] the
 * per-proof scalars and item digests, [1] hash tree, seed and z', [2] column sums and the proofs' own terms, [3] the multi-scalar
 * multiplication; -1 where there is nothing to report.
 * Out of scope: group forms, the hook into the reference (it has no such call), several generator sets per call. */
S2K_API int secp256k1_bppp_norm_product_verify_all(s2k_engine* e, int32_t* verdict, int32_t* results, unsigned char* seed32_out, const unsigned char* proofs,
                                                   size_t proof_len, const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33,
                                                   size_t n_gens, size_t g_len, const unsigned char* c_vec, size_t c_vec_len, const unsigned char* commits33, size_t n);
S2K_API int secp256k1_bppp_norm_product_verify_all_dev(s2k_engine* e, void* stream, int32_t* verdict_dev, unsigned char* seed32_out_dev, const unsigned char* proofs,
                                                       size_t proof_len, const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33_dev,
                                                       const unsigned char* gens33_host, size_t n_gens, size_t g_len, const unsigned char* c_vec, size_t c_vec_len,
                                                       const unsigned char* commits33, size_t n);
S2K_API int s2k_bppp_all_last_split_ms(s2k_engine* e, float* out4);

/* ---- `_dev` forms of the calls above (every array in HBM of the engine's GPU, stream-ordered, nothing read back) ------------------
 * Same arguments and per-item results as the host forms.  Where a call needs a few bytes on the host to plan its launches, that is
 * an explicit extra argument: gens33_host (the BP++ generator set, cache key of its fixed-base table), tally_off_host / n_pos_host
 * (the ragged tally sizes; the call returns once they have been consumed).  The half-aggregate verdict lands in result_dev[0]. */
S2K_API int secp256k1_bppp_norm_product_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* proofs, size_t proof_len,
                                                         const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33_dev,
                                                         const unsigned char* gens33_host, size_t n_gens, size_t g_len, const unsigned char* c_vec,
                                                         size_t c_vec_len, const unsigned char* commits33, size_t n);
S2K_API int secp256k1_schnorrsig_aggverify_dev(s2k_engine* e, void* stream, int32_t* result_dev, const unsigned char* pubkeys, int pk_format,
                                               const unsigned char* msgs32, size_t n, const unsigned char* aggsig, size_t aggsig_len);
/* The same with the randomizer hash's chain walked by the caller.  z_i hashes the whole prefix r_0|x(P_0)|m_0|...|m_i (main_impl.h:153-163): a
 * serial chain of 1.5 SHA-256 blocks per signature -- 118 ms on the device for 2^15 signatures, 2.6 ms on one host core with SHA extensions.
 * chain_states (HBM): ((3 n) >> 1) x 8 words, the state after every full 64-byte block behind the tag midstate; s2k_halfagg_chain_states
 * computes them from host copies of the inputs.  NULL = the plain `_dev` form (device chain).  The states are input data of the caller: a
 * wrong array gives a wrong verdict for that aggregate only. */
S2K_API int secp256k1_schnorrsig_aggverify_dev_chain(s2k_engine* e, void* stream, int32_t* result_dev, const unsigned char* pubkeys, int pk_format,
                                                     const unsigned char* msgs32, size_t n, const unsigned char* aggsig, size_t aggsig_len,
                                                     const uint32_t* chain_states);
S2K_API int s2k_halfagg_chain_states(uint32_t* states_out, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32, size_t n,
                                     const unsigned char* aggsig);
S2K_API int secp256k1_pedersen_verify_tally_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* commits33,
                                                      const uint64_t* tally_off_host, const uint64_t* n_pos_host, size_t n_tallies);
S2K_API int secp256k1_rangeproof_rewind_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* blind_out, uint64_t* value_out,
                                                  unsigned char* message_out, uint64_t* outlen, size_t msg_stride, const unsigned char* nonces,
                                                  uint64_t* min_value, uint64_t* max_value, const unsigned char* commits33, const unsigned char* proofs,
                                                  const uint64_t* proof_off, const unsigned char* extra, const uint64_t* extra_off,
                                                  const unsigned char* gens64, size_t n);

/* ---- Bulletproofs++ commitments on the fixed-base tables -----------------------------------------------
 * commits33[i] = serialize_ext( secp256k1_bppp_commit(ctx, scratch, &commit, gens, n_vec_i, g_len, l_vec_i, h_len, c_vec_i, h_len, &mu_i) )
 *              = v G + sum n_i G_i + sum l_j H_j ,  v = sum n_i^2 mu^(i+1) + <l, c>
 *                                       (static, src/modules/bppp/bppp_norm_product_impl.h:105-151; serialisation src/secp256k1.c:885-891:
 *                                        33 zero bytes = infinity)
 * gens33: n_gens = g_len + h_len compressed generators (G_i first, then H_j), shared by the batch and cached as a fixed-base table
 * like the verifier's; n_vec n*g_len*32, l_vec / c_vec n*h_len*32, mu n*32 (scalars, big-endian, reduced mod the group order).
 * results (may be NULL): 1 per item when the generator set parsed, else 0 (the reference cannot be handed an unparsed set).
 * The `_dev` form takes every array in HBM plus the generator set a second time on the host (gens33_host: the table's cache key). */
S2K_API int secp256k1_bppp_commit_batch(s2k_engine* e, unsigned char* commits33, int32_t* results, const unsigned char* gens33, size_t n_gens, size_t g_len,
                                        const unsigned char* n_vec, const unsigned char* l_vec, const unsigned char* c_vec, size_t h_len,
                                        const unsigned char* mu, size_t n);
S2K_API int secp256k1_bppp_commit_batch_dev(s2k_engine* e, void* stream, unsigned char* commits33, int32_t* results, const unsigned char* gens33_dev,
                                            const unsigned char* gens33_host, size_t n_gens, size_t g_len, const unsigned char* n_vec,
                                            const unsigned char* l_vec, const unsigned char* c_vec, size_t h_len, const unsigned char* mu, size_t n);

/* ---- engine groups: the GPUs of one node behind one handle ------------------------------------------------------------------------
 * A group holds one engine per entry of `devices` (HIP device ordinals; an ordinal may appear more than once -- engines on one device
 * share that device's tables) and one host thread per engine.  Independent items are replica work ("batches of independent
 * proofs: replicas only"): `_group` batch calls cut the batch into contiguous index ranges, one per engine, and run them concurrently
 * through the engines' host-buffer entry points; arguments, per-item results and error conventions are those of the single-engine
 * calls (a failing engine fails the call and zeroes `results`).  One LARGE multi-scalar multiplication is sharded by terms
 * (BASELINE config 5): every engine sums its slice to a 112-byte Jacobian partial, the partials are copied to the first engine's
 * device (hipMemcpyPeerAsync; devices that can reach each other over xGMI are made peers) and summed there.  s2k_ecmult_multi_group
 * takes host arrays (each engine uploads its slice); s2k_ecmult_multi_group_dev takes, per engine i, device pointers to a slice that
 * is already resident on engine i's GPU (n_per_engine[i] terms; pt_inf_dev may be NULL; g_sc_dev0: 32 bytes on engine 0's GPU or
 * NULL) -- the result comes back to the host in both.  One group call runs at a time; the engines of a group may also be used directly
 * (s2k_group_engine), e.g. to cache a generator on every device.
 * A group handle fits the reference-side hook's `engine` slot (integration/secp256k1_amd_hook.h): the `_group` functions have the
 * single-engine prototypes with the handle type changed. */
typedef struct s2k_group s2k_group;
S2K_API s2k_group* s2k_group_create(const int* devices, int n);
S2K_API void s2k_group_destroy(s2k_group* g);
S2K_API int s2k_group_size(const s2k_group* g);
S2K_API s2k_engine* s2k_group_engine(s2k_group* g, int i);
S2K_API int secp256k1_rangeproof_verify_batch_group(s2k_group* g, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                    const unsigned char* commits33, const unsigned char* proofs, const uint64_t* proof_off,
                                                    const unsigned char* extra, const uint64_t* extra_off, const unsigned char* gens64, size_t n);
S2K_API int secp256k1_rangeproof_verify_batch_ptrs_group(s2k_group* g, int32_t* results, uint64_t* min_value, uint64_t* max_value,
                                                         const void* const* commit_objs, const unsigned char* const* proofs, const size_t* plens,
                                                         const unsigned char* const* extra, const size_t* elens, const void* const* gen_objs, size_t n);
S2K_API int secp256k1_schnorrsig_verify_batch_group(s2k_group* g, int32_t* results, const unsigned char* sigs, const unsigned char* msgs,
                                                    size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_ecdsa_verify_batch_group(s2k_group* g, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                               const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n);
S2K_API int secp256k1_ecdsa_adaptor_verify_batch_group(s2k_group* g, int32_t* results, const unsigned char* adaptor_sigs162, const unsigned char* pubkeys,
                                                       const unsigned char* msgs32, const unsigned char* enckeys, int pk_format, size_t n);
S2K_API int secp256k1_ecdsa_s2c_verify_commit_batch_group(s2k_group* g, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                          const unsigned char* data32, const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_anti_exfil_host_verify_batch_group(s2k_group* g, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                         const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, const unsigned char* host_data32,
                                                         const unsigned char* openings, int opening_format, size_t n);
S2K_API int secp256k1_ellswift_decode_batch_group(s2k_group* g, unsigned char* out, int out_format, const unsigned char* ell64, size_t n);
/* (every engine gets its share of the items and the whole cache / session arrays) */
S2K_API int secp256k1_musig_partial_sig_verify_batch_group(s2k_group* g, int32_t* results, const unsigned char* partial_sigs, int sig_format,
                                                           const unsigned char* pubnonces, int nonce_format, const unsigned char* pubkeys, int pk_format,
                                                           const unsigned char* keyagg_caches197, const unsigned char* sessions133, size_t n_sessions,
                                                           const uint32_t* session_of, size_t n);
S2K_API int secp256k1_xonly_pubkey_tweak_add_check_batch_group(s2k_group* g, int32_t* results, const unsigned char* tweaked32, const unsigned char* parities,
                                                               const unsigned char* internal_keys, int key_format, const unsigned char* tweaks32, size_t n);
S2K_API int secp256k1_ec_pubkey_tweak_mul_batch_group(s2k_group* g, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                      const unsigned char* keys, int key_format, const unsigned char* tweaks32, size_t n);
S2K_API int s2k_ecmult_multi_group(s2k_group* g, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc, const unsigned char* sc,
                                   const unsigned char* pt_xy, const unsigned char* pt_inf, size_t n);
S2K_API int s2k_ecmult_multi_group_dev(s2k_group* g, unsigned char* r_xy, int32_t* r_inf, const unsigned char* g_sc_dev0,
                                       const unsigned char* const* sc_dev, const unsigned char* const* pt_xy_dev,
                                       const unsigned char* const* pt_inf_dev, const size_t* n_per_engine);

#ifdef __cplusplus
}
#endif
#endif
