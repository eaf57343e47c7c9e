#include "engine_lanes.h"
#include "s2c.h"

// ------------------------------------------------------------------------------------------------------------
// ECDSA sign-to-contract checks and anti-exfil host verification (s2c.h): one item per lane
// ------------------------------------------------------------------------------------------------------------
// (k_s2c_commit calls neither ecmult_lane nor an inversion: no per-lane table slice, no digit stream in LDS, and a lane's verdict depends
// on no other lane.  Host verification is by default a chain of two launches: k_s2c_commit leaves its verdicts in `results` and
// k_s2c_ecdsa_and, which is k_ecdsa_verify with one more line, ANDs the ECDSA verdicts into them.  k_s2c_host_verify is the fused form,
// the commitment half and then ecmult_lane in one kernel: it keeps two waves per SIMD without scratch, but measured slower than the sum
// of the chain's two kernels at 2^16 and at 2^20 items, so it runs only under S2K_OPT_S2C_FUSED.  Resource lines and rates: DESIGN.md 7.8.)
__global__ void __launch_bounds__(256, 2)
k_s2c_commit(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, const uint64_t* __restrict__ sig_off, int sig_format,
             const unsigned char* __restrict__ data32, const unsigned char* __restrict__ openings, int opening_format, s2c_midstates mid,
             const u32* __restrict__ gtab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    const unsigned char* sig = sigs + 64 * ii; u64 size = 64;
    if (sig_format == ECDSA_SIG_DER) { const u64 a = sig_off[ii], b = sig_off[ii + 1]; sig = sigs + a; size = b >= a ? b - a : 0; }
    const int r = s2c_commit_lane(mid, sig, size, sig_format, data32 + 32 * ii, openings + s2c_opening_bytes(opening_format) * ii, opening_format, live, gtab);
    if (live) results[i] = r;
}
__global__ void __launch_bounds__(256, 2)
k_s2c_host_verify(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, const uint64_t* __restrict__ sig_off, int sig_format,
                  const unsigned char* __restrict__ msgs, const unsigned char* __restrict__ pks, int pk_format, const unsigned char* __restrict__ data32,
                  const unsigned char* __restrict__ openings, int opening_format, s2c_midstates mid, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const unsigned char* sig = sigs + 64 * ii; u64 size = 64;
    if (sig_format == ECDSA_SIG_DER) { const u64 a = sig_off[ii], b = sig_off[ii + 1]; sig = sigs + a; size = b >= a ? b - a : 0; }
    const int r = s2c_host_verify_lane(mid, sig, size, sig_format, msgs + 32 * ii, pks + ecdsa_pk_bytes(pk_format) * ii, pk_format, data32 + 32 * ii,
                                       openings + s2c_opening_bytes(opening_format) * ii, opening_format, live, gtab, lm);
    if (live) results[i] = r;
}
// second kernel of the chain: results[i] &= ECDSA verdict.  Every lane walks ecmult_lane, whatever the commitment kernel found.
__global__ void __launch_bounds__(256, 2)
k_s2c_ecdsa_and(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, const uint64_t* __restrict__ sig_off, int sig_format,
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
    if (live) results[i] &= r;
}
__global__ void __launch_bounds__(256)
k_s2c_host_commit(unsigned char* __restrict__ out32, const unsigned char* __restrict__ rand32, s2c_midstates mid, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) s2c_host_commit_lane(out32 + 32 * i, mid, rand32 + 32 * i);
}

static int s2c_formats_ok(const char* who, int sig_format, int pk_format, int opening_format) {
    if (sig_format < 0 || sig_format > 2) return s2k_fail_arg(who, "sig_format must be 0 (compact), 1 (object) or 2 (DER)");
    if (pk_format < 0 || pk_format > 2) return s2k_fail_arg(who, "pk_format must be 0 (compressed), 1 (object) or 2 (uncompressed / hybrid)");
    if (opening_format < 0 || opening_format > 1) return s2k_fail_arg(who, "opening_format must be 0 (compressed, 33 bytes) or 1 (object)");
    return 1;
}

extern "C" int secp256k1_ecdsa_s2c_verify_commit_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                           int sig_format, const unsigned char* data32, const unsigned char* openings, int opening_format, size_t n) {
    const char* who = "secp256k1_ecdsa_s2c_verify_commit_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !data32 || !openings || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!s2c_formats_ok(who, sig_format, 0, opening_format)) return 0;
    s2c_midstates mid; s2c_tag_midstates(mid);                            // (four compressions on the host: not worth a field of the engine)
    const int der = sig_format == ECDSA_SIG_DER;
    const size_t ob = s2c_opening_bytes(opening_format);
    return lanes_run(e, stream, n, {true, false, 0}, {{results, sizeof(int32_t) * n}},        // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_s2c_commit, grid, dim3(256), 0, st, results + i0, der ? sigs : sigs + 64 * i0, der ? sig_off + i0 : nullptr, sig_format, data32 + 32 * i0,
                           openings + ob * i0, opening_format, mid, e->gtab, m);
    });
}

extern "C" int secp256k1_anti_exfil_host_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                          int sig_format, const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format,
                                                          const unsigned char* host_data32, const unsigned char* openings, int opening_format, size_t n) {
    const char* who = "secp256k1_anti_exfil_host_verify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msghash32 || !pubkeys || !host_data32 || !openings || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!s2c_formats_ok(who, sig_format, pk_format, opening_format)) return 0;
    s2c_midstates mid; s2c_tag_midstates(mid);
    const int der = sig_format == ECDSA_SIG_DER;
    const size_t pkb = ecdsa_pk_bytes(pk_format), ob = s2c_opening_bytes(opening_format);
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}},         // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        const unsigned char* sg = der ? sigs : sigs + 64 * i0;
        const uint64_t* so = der ? sig_off + i0 : nullptr;
        if (e->s2c_fused) {
            hipLaunchKernelGGL(k_s2c_host_verify, grid, dim3(256), 0, st, results + i0, sg, so, sig_format, msghash32 + 32 * i0, pubkeys + pkb * i0, pk_format,
                               host_data32 + 32 * i0, openings + ob * i0, opening_format, mid, e->gtab, e->ptab, m);
        } else {
            hipLaunchKernelGGL(k_s2c_commit, grid, dim3(256), 0, st, results + i0, sg, so, sig_format, host_data32 + 32 * i0, openings + ob * i0, opening_format, mid, e->gtab, m);
            hipLaunchKernelGGL(k_s2c_ecdsa_and, grid, dim3(256), 0, st, results + i0, sg, so, sig_format, msghash32 + 32 * i0, pubkeys + pkb * i0, pk_format, e->gtab, e->ptab, m);
        }
    });
}

// host form of both verifiers: msghash32 == NULL selects the commitment check alone (its callers have checked their own arguments)
static int s2c_host_form(const char* who, s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                         const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, const unsigned char* data32, const unsigned char* openings,
                         int opening_format, size_t n) {
    memset(results, 0, sizeof(int32_t) * n);
    if (!s2c_formats_ok(who, sig_format, pk_format, opening_format)) return 0;
    const int full = msghash32 != nullptr;
    der_span sw;
    if (!der_window(who, sw, sigs, sig_off, sig_format, n)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t pkb = full ? ecdsa_pk_bytes(pk_format) : 0, ob = s2c_opening_bytes(opening_format);
    stage_buf b[] = {{nullptr, results, 4 * n}, {sw.lo, nullptr, sw.bytes, 64}, {sw.rel.data(), nullptr, 8 * (n + 1)}, {msghash32, nullptr, 32 * n}, {pubkeys, nullptr, pkb * n},
                     {data32, nullptr, 32 * n}, {openings, nullptr, ob * n}};
    if (!stage_open(e, b)) return 0;
    int32_t* d_res = b[0].at<int32_t>(); const uint64_t* d_off = b[2].opt<uint64_t>();
    return stage_close(e, b, full ? secp256k1_anti_exfil_host_verify_batch_dev(e, nullptr, d_res, b[1].at(), d_off, sig_format, b[3].at(), b[4].at(), pk_format, b[5].at(), b[6].at(), opening_format, n)
                                  : secp256k1_ecdsa_s2c_verify_commit_batch_dev(e, nullptr, d_res, b[1].at(), d_off, sig_format, b[5].at(), b[6].at(), opening_format, n));
}
extern "C" int secp256k1_ecdsa_s2c_verify_commit_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                       const unsigned char* data32, const unsigned char* openings, int opening_format, size_t n) {
    const char* who = "secp256k1_ecdsa_s2c_verify_commit_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !data32 || !openings || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return s2c_host_form(who, e, results, sigs, sig_off, sig_format, nullptr, nullptr, 0, data32, openings, opening_format, n);
}
extern "C" int secp256k1_anti_exfil_host_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off, int sig_format,
                                                      const unsigned char* msghash32, const unsigned char* pubkeys, int pk_format, const unsigned char* host_data32,
                                                      const unsigned char* openings, int opening_format, size_t n) {
    const char* who = "secp256k1_anti_exfil_host_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msghash32 || !pubkeys || !host_data32 || !openings || (sig_format == ECDSA_SIG_DER && !sig_off)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return s2c_host_form(who, e, results, sigs, sig_off, sig_format, msghash32, pubkeys, pk_format, host_data32, openings, opening_format, n);
}

extern "C" int secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(s2k_engine* e, void* stream, unsigned char* commitments_out32, const unsigned char* rand32, size_t n) {
    const char* who = "secp256k1_ecdsa_anti_exfil_host_commit_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!commitments_out32 || !rand32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    s2c_midstates mid; s2c_tag_midstates(mid);
    return lanes_run(e, stream, n, {false, false, 0}, {{commitments_out32, 32 * n}}, [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_s2c_host_commit, grid, dim3(256), 0, st, commitments_out32 + 32 * i0, rand32 + 32 * i0, mid, m);
    });
}
extern "C" int secp256k1_ecdsa_anti_exfil_host_commit_batch(s2k_engine* e, unsigned char* commitments_out32, const unsigned char* rand32, size_t n) {
    const char* who = "secp256k1_ecdsa_anti_exfil_host_commit_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!commitments_out32 || !rand32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(commitments_out32, 0, 32 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, commitments_out32, 32 * n}, {rand32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(e, nullptr, b[0].at(), b[1].at(), n));
}
