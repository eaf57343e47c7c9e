#include "engine_lanes.h"
#include "ecdsa.h"

// ------------------------------------------------------------------------------------------------------------
// ECDSA batch verification and public-key recovery (ecdsa.h): one item per lane
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2)
k_ecdsa_verify(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, const uint64_t* __restrict__ sig_off, int sig_format,
               const unsigned char* __restrict__ msgs, const unsigned char* __restrict__ pks, int pk_format, const u32* __restrict__ gtab,
               u32* __restrict__ ptab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const unsigned char* sig = sigs + 64 * ii; u64 size = 64;
    if (sig_format == ECDSA_SIG_DER) { const u64 a = sig_off[ii], b = sig_off[ii + 1]; sig = sigs + a; size = b >= a ? b - a : 0; }
    const int r = ecdsa_verify_lane(sig, size, sig_format, msgs + 32 * ii, pks + ecdsa_pk_bytes(pk_format) * ii, pk_format, live, gtab, lm);
    if (live) results[i] = r;
}
// (no lane leaves early: the to-affine inversion at the end of ecdsa_recover_lane is shared by the 64 lanes of a wavefront)
__global__ void __launch_bounds__(256, 2)
k_ecdsa_recover(int32_t* __restrict__ results, unsigned char* __restrict__ pk_out, const unsigned char* __restrict__ sigs, const unsigned char* __restrict__ recids,
                const unsigned char* __restrict__ msgs, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = ecdsa_recover_lane(pk_out + 64 * ii, sigs + 64 * ii, recids[ii], msgs + 32 * ii, live, gtab, lm);
    if (live) results[i] = r;
}

static int ecdsa_formats_ok(const char* who, int sig_format, int pk_format) {
    if (sig_format < 0 || sig_format > 2) return s2k_fail_arg(who, "sig_format must be 0 (compact), 1 (object) or 2 (DER)");
    if (pk_format < 0 || pk_format > 2) return s2k_fail_arg(who, "pk_format must be 0 (compressed), 1 (object) or 2 (uncompressed / hybrid)");
    return 1;
}

extern "C" int secp256k1_ecdsa_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                int sig_format, const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n) {
    const char* who = "secp256k1_ecdsa_verify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msghash32 || !pubkeys || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!ecdsa_formats_ok(who, sig_format, pk_format)) return 0;
    const int der = sig_format == ECDSA_SIG_DER;
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}},         // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_ecdsa_verify, grid, dim3(256), 0, st, results + i0, der ? sigs : sigs + 64 * i0, der ? sig_off + i0 : nullptr, sig_format,
                           msghash32 + 32 * i0, pubkeys + pkb * i0, pk_format, e->gtab, e->ptab, m);
    });
}
extern "C" int secp256k1_ecdsa_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                            const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n) {
    const char* who = "secp256k1_ecdsa_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msghash32 || !pubkeys || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (!ecdsa_formats_ok(who, sig_format, pk_format)) return 0;
    der_span sw;
    if (!der_window(who, sw, sigs, sig_off, sig_format, n)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    stage_buf b[] = {{nullptr, results, 4 * n}, {sw.lo, nullptr, sw.bytes, 64}, {sw.rel.data(), nullptr, 8 * (n + 1)}, {msghash32, nullptr, 32 * n}, {pubkeys, nullptr, pkb * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ecdsa_verify_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].opt<uint64_t>(), sig_format, b[3].at(),
                                                              b[4].at(), pk_format, n));
}

extern "C" int secp256k1_ecdsa_recover_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* sigs64,
                                                 const unsigned char* recids, const unsigned char* msghash32, size_t n) {
    const char* who = "secp256k1_ecdsa_recover_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !pubkeys_out64 || !sigs64 || !recids || !msghash32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}, {pubkeys_out64, 64 * n}},       // a batch that does not complete shows no item as recovered
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_ecdsa_recover, grid, dim3(256), 0, st, results + i0, pubkeys_out64 + 64 * i0, sigs64 + 64 * i0, recids + i0, msghash32 + 32 * i0,
                           e->gtab, e->ptab, m);
    });
}
extern "C" int secp256k1_ecdsa_recover_batch(s2k_engine* e, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* sigs64,
                                             const unsigned char* recids, const unsigned char* msghash32, size_t n) {
    const char* who = "secp256k1_ecdsa_recover_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !pubkeys_out64 || !sigs64 || !recids || !msghash32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(pubkeys_out64, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, pubkeys_out64, 64 * n}, {sigs64, nullptr, 64 * n}, {recids, nullptr, n, 64}, {msghash32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ecdsa_recover_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].at(), b[4].at(), n));
}
