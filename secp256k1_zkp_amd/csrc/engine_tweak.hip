#include "engine_lanes.h"
#include "tweak.h"

// ------------------------------------------------------------------------------------------------------------
// Taproot tweak checks and public-key tweak-add (tweak.h): one item per lane
// ------------------------------------------------------------------------------------------------------------
// (no lane leaves early: the to-affine inversion in tweak_affine_lane is shared by the 64 lanes of a wavefront.  Neither kernel calls
// ecmult_lane: no per-lane table slice and no digit stream in LDS.  Two waves per SIMD is the most the compiler reaches without scratch
// (182 / 178 VGPRs); -DS2K_TWEAK_WAVES=3 builds the 168-register variant, which spills 44 / 32 bytes per lane.)
#ifndef S2K_TWEAK_WAVES
#define S2K_TWEAK_WAVES 2
#endif
__global__ void __launch_bounds__(256, S2K_TWEAK_WAVES)
k_tweak_check(int32_t* __restrict__ results, const unsigned char* __restrict__ tweaked32, const unsigned char* __restrict__ parities,
              const unsigned char* __restrict__ keys, int key_format, const unsigned char* __restrict__ tweaks32, const u32* __restrict__ gtab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    const int r = tweak_check_lane(tweaked32 + 32 * ii, parities[ii], keys + tweak_key_bytes(key_format) * ii, key_format, tweaks32 + 32 * ii, live, gtab);
    if (live) results[i] = r;
}
__global__ void __launch_bounds__(256, S2K_TWEAK_WAVES)
k_tweak_add(int32_t* __restrict__ results, unsigned char* __restrict__ pk_out, const unsigned char* __restrict__ keys, int key_format,
            const unsigned char* __restrict__ tweaks32, const u32* __restrict__ gtab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    const int r = tweak_add_lane(pk_out + 64 * ii, keys + tweak_key_bytes(key_format) * ii, key_format, tweaks32 + 32 * ii, live, gtab);
    if (live) results[i] = r;
}

extern "C" int secp256k1_xonly_pubkey_tweak_add_check_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* tweaked32,
                                                                const unsigned char* parities, const unsigned char* internal_keys, int key_format,
                                                                const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_xonly_pubkey_tweak_add_check_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !tweaked32 || !parities || !internal_keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (key_format < 0 || key_format > 1) return s2k_fail_arg(who, "key_format must be 0 (x-only, 32 bytes) or 1 (object)");
    const size_t kb = tweak_key_bytes(key_format);
    return lanes_run(e, stream, n, {true, false, 0}, {{results, sizeof(int32_t) * n}},        // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_tweak_check, grid, dim3(256), 0, st, results + i0, tweaked32 + 32 * i0, parities + i0, internal_keys + kb * i0, key_format,
                           tweaks32 + 32 * i0, e->gtab, m);
    });
}
extern "C" int secp256k1_xonly_pubkey_tweak_add_check_batch(s2k_engine* e, int32_t* results, const unsigned char* tweaked32, const unsigned char* parities,
                                                            const unsigned char* internal_keys, int key_format, const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_xonly_pubkey_tweak_add_check_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !tweaked32 || !parities || !internal_keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (key_format < 0 || key_format > 1) return s2k_fail_arg(who, "key_format must be 0 (x-only, 32 bytes) or 1 (object)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t kb = tweak_key_bytes(key_format);
    stage_buf b[] = {{nullptr, results, 4 * n}, {tweaked32, nullptr, 32 * n}, {parities, nullptr, n, 64}, {internal_keys, nullptr, kb * n}, {tweaks32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_xonly_pubkey_tweak_add_check_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].at(), key_format, b[4].at(), n));
}

extern "C" int secp256k1_pubkey_tweak_add_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* keys,
                                                    int key_format, const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_pubkey_tweak_add_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !pubkeys_out64 || !keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (key_format < 0 || key_format > 2) return s2k_fail_arg(who, "key_format must be 0 (x-only, 32 bytes), 1 (object) or 2 (compressed)");
    const size_t kb = tweak_key_bytes(key_format);
    return lanes_run(e, stream, n, {true, false, 0}, {{results, sizeof(int32_t) * n}, {pubkeys_out64, 64 * n}},      // a batch that does not complete shows no item as tweaked
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_tweak_add, grid, dim3(256), 0, st, results + i0, pubkeys_out64 + 64 * i0, keys + kb * i0, key_format, tweaks32 + 32 * i0, e->gtab, m);
    });
}
extern "C" int secp256k1_pubkey_tweak_add_batch(s2k_engine* e, int32_t* results, unsigned char* pubkeys_out64, const unsigned char* keys, int key_format,
                                                const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_pubkey_tweak_add_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !pubkeys_out64 || !keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(pubkeys_out64, 0, 64 * n);
    if (key_format < 0 || key_format > 2) return s2k_fail_arg(who, "key_format must be 0 (x-only, 32 bytes), 1 (object) or 2 (compressed)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t kb = tweak_key_bytes(key_format);
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, pubkeys_out64, 64 * n}, {keys, nullptr, kb * n, 64}, {tweaks32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_pubkey_tweak_add_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), key_format, b[3].at(), n));
}
