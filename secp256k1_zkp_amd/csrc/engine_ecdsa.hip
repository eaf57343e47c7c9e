#include "engine_internal.h"
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
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!engine_ptab(e, ((std::min(n, e->max_lanes) + 255) / 256) * 256)) return 0;
    ENGINE_GTAB(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete never shows an item as valid
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_ecdsa_verify, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, sig_format == ECDSA_SIG_DER ? sigs : sigs + 64 * i0,
                           sig_format == ECDSA_SIG_DER ? sig_off + i0 : nullptr, sig_format, msghash32 + 32 * i0, pubkeys + pkb * i0, pk_format, e->gtab, e->ptab, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_ecdsa_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                            const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, size_t n) {
    const char* who = "secp256k1_ecdsa_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msghash32 || !pubkeys || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (!ecdsa_formats_ok(who, sig_format, pk_format)) return 0;
    const int der = sig_format == ECDSA_SIG_DER;
    if (der) for (size_t i = 0; i < n; i++) if (sig_off[i + 1] < sig_off[i]) return s2k_fail_arg(who, "sig_off must not decrease");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    // DER: the items' bytes [sig_off[0], sig_off[n]) go to HBM as they are; the offsets stay the caller's, the base pointer moves back
    const size_t sig_lo = der ? (size_t)sig_off[0] : 0, sig_bytes = der ? (size_t)(sig_off[n] - sig_off[0]) : 64 * n, pkb = ecdsa_pk_bytes(pk_format);
    if (!engine_workspace(e, ws_need({4 * n, sig_bytes + 64, 8 * (n + 1), 32 * n, pkb * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_sig = w.take<unsigned char>(sig_bytes + 64); uint64_t* d_off = w.take<uint64_t>(n + 1);
    unsigned char* d_msg = w.take<unsigned char>(32 * n); unsigned char* d_pk = w.take<unsigned char>(pkb * n);
    std::vector<uint64_t> rel;
    if (sig_bytes) HIPCHK(hipMemcpyAsync(d_sig, sigs + sig_lo, sig_bytes, hipMemcpyHostToDevice, e->stream));
    if (der) {
        rel.resize(n + 1);
        for (size_t i = 0; i <= n; i++) rel[i] = sig_off[i] - sig_lo;
        HIPCHK(hipMemcpyAsync(d_off, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipMemcpyAsync(d_msg, msghash32, 32 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_pk, pubkeys, pkb * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_ecdsa_verify_batch_dev(e, nullptr, d_res, d_sig, der ? d_off : nullptr, sig_format, d_msg, d_pk, pk_format, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

extern "C" int secp256k1_ecdsa_recover_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* sigs64,
                                                 const unsigned char* recids, const unsigned char* msghash32, size_t n) {
    const char* who = "secp256k1_ecdsa_recover_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !pubkeys_out64 || !sigs64 || !recids || !msghash32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!engine_ptab(e, ((std::min(n, e->max_lanes) + 255) / 256) * 256)) return 0;
    ENGINE_GTAB(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete shows no item as recovered
    HIPCHK(hipMemsetAsync(pubkeys_out64, 0, 64 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_ecdsa_recover, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, pubkeys_out64 + 64 * i0, sigs64 + 64 * i0, recids + i0,
                           msghash32 + 32 * i0, e->gtab, e->ptab, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
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
    if (!engine_workspace(e, ws_need({4 * n, 64 * n, 64 * n, n + 64, 32 * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_pk = w.take<unsigned char>(64 * n); unsigned char* d_sig = w.take<unsigned char>(64 * n);
    unsigned char* d_id = w.take<unsigned char>(n + 64); unsigned char* d_msg = w.take<unsigned char>(32 * n);
    HIPCHK(hipMemcpyAsync(d_sig, sigs64, 64 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_id, recids, n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_msg, msghash32, 32 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_ecdsa_recover_batch_dev(e, nullptr, d_res, d_pk, d_sig, d_id, d_msg, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(pubkeys_out64, d_pk, 64 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}
