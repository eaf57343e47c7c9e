#include "engine_internal.h"
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
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const size_t ob = ellswift_out_bytes(out_format);
    HIPCHK(hipMemsetAsync(out, 0, ob * n, st));                           // a batch that does not complete leaves no stale key behind
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_ellswift_decode, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out + ob * i0, out_format, ell64 + 64 * i0, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
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
    if (!engine_workspace(e, ws_need({ob * n, 64 * n}))) return 0;
    ws_carver w{e->ws, 0};
    unsigned char* d_out = w.take<unsigned char>(ob * n); unsigned char* d_in = w.take<unsigned char>(64 * n);
    HIPCHK(hipMemcpyAsync(d_in, ell64, 64 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_ellswift_decode_batch_dev(e, nullptr, d_out, out_format, d_in, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(out, d_out, ob * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

extern "C" int secp256k1_ellswift_encode_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* ell64_out, const unsigned char* keys, int key_format,
                                                   const unsigned char* rnd32, size_t n) {
    const char* who = "secp256k1_ellswift_encode_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !ell64_out || !keys || !rnd32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (key_format < 1 || key_format > 2) return s2k_fail_arg(who, "key_format must be 1 (n*64 objects) or 2 (n*33 compressed)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    ellswift_midstate mid; ellswift_tag_midstate(mid);                    // (two compressions on the host: not worth a field of the engine)
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete shows no item as encoded
    HIPCHK(hipMemsetAsync(ell64_out, 0, 64 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    const size_t kb = tweak_key_bytes(key_format);
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_ellswift_encode, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, ell64_out + 64 * i0, keys + kb * i0, key_format,
                           rnd32 + 32 * i0, mid, (u32)e->ellswift_max_attempts, e->dev_flags + 1, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
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
    if (!engine_workspace(e, ws_need({4 * n, 64 * n, kb * n, 32 * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_out = w.take<unsigned char>(64 * n); unsigned char* d_key = w.take<unsigned char>(kb * n);
    unsigned char* d_rnd = w.take<unsigned char>(32 * n);
    HIPCHK(hipMemcpyAsync(d_key, keys, kb * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_rnd, rnd32, 32 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_ellswift_encode_batch_dev(e, nullptr, d_res, d_out, d_key, key_format, d_rnd, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(ell64_out, d_out, 64 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
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
