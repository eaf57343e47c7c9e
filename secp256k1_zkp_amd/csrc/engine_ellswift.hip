#include "engine_lanes.h"
#include "ellswift.h"

// ------------------------------------------------------------------------------------------------------------
// ElligatorSwift decoding and encoding (ellswift.h): one item per lane
// ------------------------------------------------------------------------------------------------------------
// (no lane leaves early in either kernel: the inversion of the decode and the one inside every round of the encode are shared by the
// 64 lanes of a wavefront; a lane without an item reads item 0 and hands 1 to the inversion.  out_format and key_format are the same
// for every lane of a launch.  k_ellswift_encode is the plain form of the loop: a wavefront runs as many rounds as the slowest of its
// items needs, at most max_attempts.  Resource lines and rates: DESIGN.md 7.9.)
__global__ void __launch_bounds__(256, 2)
k_ellswift_decode(unsigned char* __restrict__ out, int out_format, const unsigned char* __restrict__ ell64, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    ellswift_decode_lane(out + ellswift_out_bytes(out_format) * ii, out_format, ell64 + 64 * ii, live);
}
__global__ void __launch_bounds__(256, 2)
k_ellswift_encode(int32_t* __restrict__ results, unsigned char* __restrict__ ell64_out, const unsigned char* __restrict__ keys, int key_format,
                  const unsigned char* __restrict__ rnd32, ellswift_midstate mid, u32 max_attempts, u32* __restrict__ capped_count, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    int capped = 0;
    const int r = ellswift_encode_lane(ell64_out + 64 * ii, &capped, mid, keys + tweak_key_bytes(key_format) * ii, key_format, rnd32 + 32 * ii, live, max_attempts);
    if (live) results[i] = r;
    if (live && capped) atomicAdd(capped_count, 1u);              // (out of reach of any input at the default cap: see ELLSWIFT_MAX_ATTEMPTS)
}

extern "C" int secp256k1_ellswift_decode_batch_dev(s2k_engine* e, void* stream, unsigned char* out, int out_format, const unsigned char* ell64, size_t n) {
    const char* who = "secp256k1_ellswift_decode_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out || !ell64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (out_format < 0 || out_format > 2) return s2k_fail_arg(who, "out_format must be 0 (n*32 x only), 1 (n*64 objects) or 2 (n*33 compressed)");
    const size_t ob = ellswift_out_bytes(out_format);
    return lanes_run(e, stream, n, {false, false, 0}, {{out, ob * n}},                         // a batch that does not complete leaves no stale key behind
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_ellswift_decode, grid, dim3(256), 0, st, out + ob * i0, out_format, ell64 + 64 * i0, m);
    });
}
extern "C" int secp256k1_ellswift_decode_batch(s2k_engine* e, unsigned char* out, int out_format, const unsigned char* ell64, size_t n) {
    const char* who = "secp256k1_ellswift_decode_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out || !ell64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (out_format < 0 || out_format > 2) return s2k_fail_arg(who, "out_format must be 0 (n*32 x only), 1 (n*64 objects) or 2 (n*33 compressed)");
    const size_t ob = ellswift_out_bytes(out_format);
    memset(out, 0, ob * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, out, ob * n}, {ell64, nullptr, 64 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ellswift_decode_batch_dev(e, nullptr, b[0].at(), out_format, b[1].at(), n));
}

extern "C" int secp256k1_ellswift_encode_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* ell64_out, const unsigned char* keys, int key_format,
                                                   const unsigned char* rnd32, size_t n) {
    const char* who = "secp256k1_ellswift_encode_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !ell64_out || !keys || !rnd32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (key_format < 1 || key_format > 2) return s2k_fail_arg(who, "key_format must be 1 (n*64 objects) or 2 (n*33 compressed)");
    ellswift_midstate mid; ellswift_tag_midstate(mid);                    // (two compressions on the host: not worth a field of the engine)
    const size_t kb = tweak_key_bytes(key_format);
    return lanes_run(e, stream, n, {false, false, 0}, {{results, sizeof(int32_t) * n}, {ell64_out, 64 * n}},       // a batch that does not complete shows no item as encoded
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_ellswift_encode, grid, dim3(256), 0, st, results + i0, ell64_out + 64 * i0, keys + kb * i0, key_format, rnd32 + 32 * i0, mid,
                           (u32)e->ellswift_max_attempts, e->dev_flags + 1, m);
    });
}
extern "C" int secp256k1_ellswift_encode_batch(s2k_engine* e, int32_t* results, unsigned char* ell64_out, const unsigned char* keys, int key_format,
                                               const unsigned char* rnd32, size_t n) {
    const char* who = "secp256k1_ellswift_encode_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !ell64_out || !keys || !rnd32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (key_format < 1 || key_format > 2) return s2k_fail_arg(who, "key_format must be 1 (n*64 objects) or 2 (n*33 compressed)");
    memset(results, 0, sizeof(int32_t) * n); memset(ell64_out, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t kb = tweak_key_bytes(key_format);
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, ell64_out, 64 * n}, {keys, nullptr, kb * n}, {rnd32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ellswift_encode_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), key_format, b[3].at(), n));
}

// How many items of this engine's encode calls have hit the attempt cap since the engine was created (they got results[i] = 0 and
// zero bytes, like a refused key).  An administrative call: it waits for the device.
extern "C" int s2k_engine_ellswift_capped(s2k_engine* e, uint64_t* count) {
    const char* who = "s2k_engine_ellswift_capped";
    if (!e) return s2k_fail(who, "null engine");
    if (!count) return s2k_fail_arg(who, "illegal argument");
    *count = 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipDeviceSynchronize());
    u32 v = 0;
    HIPCHK(hipMemcpy(&v, e->dev_flags + 1, 4, hipMemcpyDeviceToHost));
    *count = v;
    return 1;
}
