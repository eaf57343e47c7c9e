#include "engine_lanes.h"
#include "musig.h"

// ------------------------------------------------------------------------------------------------------------
// MuSig2, the coordinator's half (musig.h): batch partial-signature verification and nonce processing, one item per lane
// ------------------------------------------------------------------------------------------------------------
// Both kernels park a point between two stages (musig.h), in the parking area behind the per-lane tables (engine_lanes.h: park_lanes).

// (no lane leaves early: ecmult_lane2 votes over the wavefront)
__global__ void __launch_bounds__(256, 2)
k_musig_partial_verify(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, int sig_format, const unsigned char* __restrict__ nonces, int nonce_format,
                       const unsigned char* __restrict__ pks, int pk_format, const unsigned char* __restrict__ caches, const unsigned char* __restrict__ sessions,
                       size_t n_sessions, const u32* __restrict__ session_of, musig_midstates mid, const u32* __restrict__ gtab, u32* __restrict__ ptab,
                       u32* __restrict__ park, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = musig_verify_lane(mid, sigs, sig_format, nonces, nonce_format, pks, pk_format, caches, sessions, n_sessions, session_of, ii, live, gtab, lm, park, i,
                                    (size_t)gridDim.x * blockDim.x);
    if (live) results[i] = r;
}

// (no lane leaves early: the to-affine inversions inside musig_process_lane are shared by the 64 lanes of a wavefront; HAS_ADAPTOR = 0
// has no first inversion at all)
template <int HAS_ADAPTOR>
__global__ void __launch_bounds__(256, 2)
k_musig_nonce_process(int32_t* __restrict__ results, unsigned char* sessions_out, const unsigned char* __restrict__ aggnonces, int nonce_format,
                      const unsigned char* __restrict__ msgs, const unsigned char* __restrict__ caches, const unsigned char* __restrict__ adaptors, musig_midstates mid,
                      const u32* __restrict__ gtab, u32* __restrict__ ptab, u32* __restrict__ park, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = musig_process_lane<HAS_ADAPTOR>(mid, sessions_out, aggnonces, nonce_format, msgs, caches, adaptors, ii, live, gtab, lm, park, i, (size_t)gridDim.x * blockDim.x);
    if (live) results[i] = r;
}

static int musig_formats_ok(const char* who, int sig_format, int nonce_format, int pk_format) {
    if (sig_format < 0 || sig_format > 1) return s2k_fail_arg(who, "sig_format must be 0 (32 bytes serialised) or 1 (36-byte object)");
    if (nonce_format < 0 || nonce_format > 1) return s2k_fail_arg(who, "nonce_format must be 0 (66 bytes serialised) or 1 (132-byte object)");
    if (pk_format < 0 || pk_format > 2) return s2k_fail_arg(who, "pk_format must be 0 (compressed), 1 (object) or 2 (uncompressed / hybrid)");
    return 1;
}

extern "C" int secp256k1_musig_partial_sig_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* partial_sigs, int sig_format,
                                                            const unsigned char* pubnonces, int nonce_format, const unsigned char* pubkeys, int pk_format,
                                                            const unsigned char* keyagg_caches197, const unsigned char* sessions133, size_t n_sessions,
                                                            const uint32_t* session_of, size_t n) {
    const char* who = "secp256k1_musig_partial_sig_verify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !partial_sigs || !pubnonces || !pubkeys || !keyagg_caches197 || !sessions133) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!musig_formats_ok(who, sig_format, nonce_format, pk_format)) return 0;
    if (n_sessions == 0 || (!session_of && n_sessions != n)) return s2k_fail_arg(who, "n_sessions must be n when session_of is NULL, and never 0");
    musig_midstates mid; musig_tag_midstates(mid);                        // (six compressions on the host: not worth a field of the engine)
    const size_t sgb = musig_sig_bytes(sig_format), nb = musig_nonce_bytes(nonce_format), pkb = ecdsa_pk_bytes(pk_format);
    return lanes_run(e, stream, n, {true, true, S2K_MUSIG_PARK_WORDS}, {{results, sizeof(int32_t) * n}},      // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32* park) {
        // without session_of item i uses pair i: the pair arrays move with the sub-range, and the pairs left are n_sessions - i0
        hipLaunchKernelGGL(k_musig_partial_verify, grid, dim3(256), 0, st, results + i0, partial_sigs + sgb * i0, sig_format, pubnonces + nb * i0, nonce_format,
                           pubkeys + pkb * i0, pk_format, session_of ? keyagg_caches197 : keyagg_caches197 + (size_t)MUSIG_CACHE_BYTES * i0,
                           session_of ? sessions133 : sessions133 + (size_t)MUSIG_SESSION_BYTES * i0, session_of ? n_sessions : n_sessions - i0,
                           session_of ? session_of + i0 : nullptr, mid, e->gtab, e->ptab, park, m);
    });
}
extern "C" int secp256k1_musig_partial_sig_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* partial_sigs, int sig_format, const unsigned char* pubnonces,
                                                        int nonce_format, const unsigned char* pubkeys, int pk_format, const unsigned char* keyagg_caches197,
                                                        const unsigned char* sessions133, size_t n_sessions, const uint32_t* session_of, size_t n) {
    const char* who = "secp256k1_musig_partial_sig_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !partial_sigs || !pubnonces || !pubkeys || !keyagg_caches197 || !sessions133) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (!musig_formats_ok(who, sig_format, nonce_format, pk_format)) return 0;
    if (n_sessions == 0 || (!session_of && n_sessions != n)) return s2k_fail_arg(who, "n_sessions must be n when session_of is NULL, and never 0");
    if (session_of) for (size_t i = 0; i < n; i++) if (session_of[i] >= n_sessions) return s2k_fail_arg(who, "session_of holds an index >= n_sessions");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t sgb = musig_sig_bytes(sig_format), nb = musig_nonce_bytes(nonce_format), pkb = ecdsa_pk_bytes(pk_format);
    const size_t cb = (size_t)MUSIG_CACHE_BYTES * n_sessions, sb = (size_t)MUSIG_SESSION_BYTES * n_sessions;
    stage_buf b[] = {{nullptr, results, 4 * n}, {session_of, nullptr, 4 * n}, {partial_sigs, nullptr, sgb * n}, {pubnonces, nullptr, nb * n}, {pubkeys, nullptr, pkb * n},
                     {keyagg_caches197, nullptr, cb}, {sessions133, nullptr, sb}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_musig_partial_sig_verify_batch_dev(e, nullptr, b[0].at<int32_t>(), b[2].at(), sig_format, b[3].at(), nonce_format, b[4].at(), pk_format,
                                                                          b[5].at(), b[6].at(), n_sessions, b[1].opt<uint32_t>(), n));
}

extern "C" int secp256k1_musig_nonce_process_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* sessions_out133, const unsigned char* aggnonces,
                                                       int nonce_format, const unsigned char* msgs32, const unsigned char* keyagg_caches197,
                                                       const unsigned char* adaptors64, size_t n) {
    const char* who = "secp256k1_musig_nonce_process_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sessions_out133 || !aggnonces || !msgs32 || !keyagg_caches197) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (nonce_format < 0 || nonce_format > 1) return s2k_fail_arg(who, "nonce_format must be 0 (66 bytes serialised) or 1 (132-byte object)");
    musig_midstates mid; musig_tag_midstates(mid);
    const size_t nb = musig_nonce_bytes(nonce_format);
    return lanes_run(e, stream, n, {true, true, S2K_MUSIG_PARK_R1_WORDS}, {{results, sizeof(int32_t) * n}, {sessions_out133, (size_t)MUSIG_SESSION_BYTES * n}},
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32* park) {
        if (adaptors64)
            hipLaunchKernelGGL(k_musig_nonce_process<1>, grid, dim3(256), 0, st, results + i0, sessions_out133 + (size_t)MUSIG_SESSION_BYTES * i0, aggnonces + nb * i0,
                               nonce_format, msgs32 + 32 * i0, keyagg_caches197 + (size_t)MUSIG_CACHE_BYTES * i0, adaptors64 + 64 * i0, mid, e->gtab, e->ptab, park, m);
        else
            hipLaunchKernelGGL(k_musig_nonce_process<0>, grid, dim3(256), 0, st, results + i0, sessions_out133 + (size_t)MUSIG_SESSION_BYTES * i0, aggnonces + nb * i0,
                               nonce_format, msgs32 + 32 * i0, keyagg_caches197 + (size_t)MUSIG_CACHE_BYTES * i0, (const unsigned char*)nullptr, mid, e->gtab, e->ptab, park, m);
    });
}
extern "C" int secp256k1_musig_nonce_process_batch(s2k_engine* e, int32_t* results, unsigned char* sessions_out133, const unsigned char* aggnonces, int nonce_format,
                                                   const unsigned char* msgs32, const unsigned char* keyagg_caches197, const unsigned char* adaptors64, size_t n) {
    const char* who = "secp256k1_musig_nonce_process_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sessions_out133 || !aggnonces || !msgs32 || !keyagg_caches197) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    memset(sessions_out133, 0, (size_t)MUSIG_SESSION_BYTES * n);
    if (nonce_format < 0 || nonce_format > 1) return s2k_fail_arg(who, "nonce_format must be 0 (66 bytes serialised) or 1 (132-byte object)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t nb = musig_nonce_bytes(nonce_format), cb = (size_t)MUSIG_CACHE_BYTES * n, sb = (size_t)MUSIG_SESSION_BYTES * n;
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, sessions_out133, sb}, {aggnonces, nullptr, nb * n}, {msgs32, nullptr, 32 * n}, {keyagg_caches197, nullptr, cb},
                     {adaptors64, nullptr, 64 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_musig_nonce_process_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), nonce_format, b[3].at(), b[4].at(), b[5].opt(), n));
}
