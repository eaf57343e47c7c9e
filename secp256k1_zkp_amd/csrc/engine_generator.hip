#include "engine_internal.h"
#include "generator.h"

// ------------------------------------------------------------------------------------------------------------
// Asset generators and explicit-amount commitments (generator.h): one item per lane
// ------------------------------------------------------------------------------------------------------------
// (no lane leaves early in k_gen_generate and k_pedersen_commit: their inversions are shared by the 64 lanes of a wavefront.  blinds32
// is NULL or not for a whole launch, so the fixed-base part is a uniform branch.)
__global__ void __launch_bounds__(256, 2)
k_gen_generate(int32_t* __restrict__ results, unsigned char* __restrict__ gens_out, const unsigned char* __restrict__ keys32,
               const unsigned char* __restrict__ blinds32, const u32* __restrict__ gtab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    const int r = generator_generate_lane(gens_out + 64 * ii, keys32 + 32 * ii, blinds32 ? blinds32 + 32 * ii : nullptr, live, gtab);
    if (live) results[i] = r;
}
// (parse and serialize share nothing across lanes: no occupancy bound is asked for; the compiler reaches 3 and 4 waves per SIMD)
__global__ void __launch_bounds__(256)
k_gen_parse(int32_t* __restrict__ results, unsigned char* __restrict__ gens_out, const unsigned char* __restrict__ gens33, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    results[i] = generator_parse_lane(gens_out + 64 * i, gens33 + 33 * i, 1);
}
__global__ void __launch_bounds__(256)
k_gen_serialize(unsigned char* __restrict__ out33, const unsigned char* __restrict__ gens64, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    generator_serialize_lane(out33 + 33 * i, gens64 + 64 * i, 1);
}
__global__ void __launch_bounds__(256, 2)
k_pedersen_commit(int32_t* __restrict__ results, unsigned char* __restrict__ commits_out, const unsigned char* __restrict__ blinds32,
                  const uint64_t* __restrict__ values, const unsigned char* __restrict__ gens64, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = pedersen_commit_lane(commits_out + 33 * ii, blinds32 ? blinds32 + 32 * ii : nullptr, values[ii], gens64 + 64 * ii, live, gtab, lm);
    if (live) results[i] = r;
}

// ---- secp256k1_generator_generate / _generate_blinded -----------------------------------------------------------------------------
extern "C" int secp256k1_generator_generate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* gens_out64, const unsigned char* keys32,
                                                      const unsigned char* blinds32, size_t n) {
    const char* who = "secp256k1_generator_generate_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !keys32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    ENGINE_GTAB(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete shows no item as generated
    HIPCHK(hipMemsetAsync(gens_out64, 0, 64 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_gen_generate, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, gens_out64 + 64 * i0, keys32 + 32 * i0,
                           blinds32 ? blinds32 + 32 * i0 : nullptr, e->gtab, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_generator_generate_batch(s2k_engine* e, int32_t* results, unsigned char* gens_out64, const unsigned char* keys32,
                                                  const unsigned char* blinds32, size_t n) {
    const char* who = "secp256k1_generator_generate_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !keys32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(gens_out64, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    if (!engine_workspace(e, ws_need({4 * n, 64 * n, 32 * n, 32 * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_gen = w.take<unsigned char>(64 * n); unsigned char* d_key = w.take<unsigned char>(32 * n);
    unsigned char* d_bl = w.take<unsigned char>(32 * n);
    HIPCHK(hipMemcpyAsync(d_key, keys32, 32 * n, hipMemcpyHostToDevice, e->stream));
    if (blinds32) HIPCHK(hipMemcpyAsync(d_bl, blinds32, 32 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_generator_generate_batch_dev(e, nullptr, d_res, d_gen, d_key, blinds32 ? d_bl : nullptr, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(gens_out64, d_gen, 64 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

// ---- secp256k1_generator_parse ----------------------------------------------------------------------------------------------------
extern "C" int secp256k1_generator_parse_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n) {
    const char* who = "secp256k1_generator_parse_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !gens33) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete shows no item as parsed
    HIPCHK(hipMemsetAsync(gens_out64, 0, 64 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_gen_parse, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, gens_out64 + 64 * i0, gens33 + 33 * i0, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_generator_parse_batch(s2k_engine* e, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n) {
    const char* who = "secp256k1_generator_parse_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !gens33) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(gens_out64, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    if (!engine_workspace(e, ws_need({4 * n, 64 * n, 33 * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_gen = w.take<unsigned char>(64 * n); unsigned char* d_in = w.take<unsigned char>(33 * n);
    HIPCHK(hipMemcpyAsync(d_in, gens33, 33 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_generator_parse_batch_dev(e, nullptr, d_res, d_gen, d_in, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(gens_out64, d_gen, 64 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

// ---- secp256k1_generator_serialize ------------------------------------------------------------------------------------------------
extern "C" int secp256k1_generator_serialize_batch_dev(s2k_engine* e, void* stream, unsigned char* out33, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_generator_serialize_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out33 || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    HIPCHK(hipMemsetAsync(out33, 0, 33 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_gen_serialize, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out33 + 33 * i0, gens64 + 64 * i0, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_generator_serialize_batch(s2k_engine* e, unsigned char* out33, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_generator_serialize_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out33 || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(out33, 0, 33 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    if (!engine_workspace(e, ws_need({33 * n, 64 * n}))) return 0;
    ws_carver w{e->ws, 0};
    unsigned char* d_out = w.take<unsigned char>(33 * n); unsigned char* d_gen = w.take<unsigned char>(64 * n);
    HIPCHK(hipMemcpyAsync(d_gen, gens64, 64 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_generator_serialize_batch_dev(e, nullptr, d_out, d_gen, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(out33, d_out, 33 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

// ---- secp256k1_pedersen_commit ----------------------------------------------------------------------------------------------------
extern "C" int secp256k1_pedersen_commit_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* commits_out33, const unsigned char* blinds32,
                                                   const uint64_t* values, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_pedersen_commit_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !commits_out33 || !values || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!engine_ptab(e, ((std::min(n, e->max_lanes) + 255) / 256) * 256)) return 0;
    ENGINE_GTAB(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete shows no item as committed
    HIPCHK(hipMemsetAsync(commits_out33, 0, 33 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_pedersen_commit, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, commits_out33 + 33 * i0,
                           blinds32 ? blinds32 + 32 * i0 : nullptr, values + i0, gens64 + 64 * i0, e->gtab, e->ptab, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_pedersen_commit_batch(s2k_engine* e, int32_t* results, unsigned char* commits_out33, const unsigned char* blinds32,
                                               const uint64_t* values, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_pedersen_commit_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !commits_out33 || !values || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(commits_out33, 0, 33 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    if (!engine_workspace(e, ws_need({4 * n, 33 * n, 32 * n, 8 * n, 64 * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_out = w.take<unsigned char>(33 * n); unsigned char* d_bl = w.take<unsigned char>(32 * n);
    uint64_t* d_val = w.take<uint64_t>(n); unsigned char* d_gen = w.take<unsigned char>(64 * n);
    if (blinds32) HIPCHK(hipMemcpyAsync(d_bl, blinds32, 32 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_val, values, 8 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_gen, gens64, 64 * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_pedersen_commit_batch_dev(e, nullptr, d_res, d_out, blinds32 ? d_bl : nullptr, d_val, d_gen, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(commits_out33, d_out, 33 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}
