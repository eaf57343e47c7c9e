#include "engine_lanes.h"
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
    return lanes_run(e, stream, n, {true, false, 0}, {{results, sizeof(int32_t) * n}, {gens_out64, 64 * n}},       // a batch that does not complete shows no item as generated
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_gen_generate, grid, dim3(256), 0, st, results + i0, gens_out64 + 64 * i0, keys32 + 32 * i0, blinds32 ? blinds32 + 32 * i0 : nullptr, e->gtab, m);
    });
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
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, gens_out64, 64 * n}, {keys32, nullptr, 32 * n}, {blinds32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_generator_generate_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].opt(), n));
}

// ---- secp256k1_generator_parse ----------------------------------------------------------------------------------------------------
extern "C" int secp256k1_generator_parse_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n) {
    const char* who = "secp256k1_generator_parse_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !gens33) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return lanes_run(e, stream, n, {false, false, 0}, {{results, sizeof(int32_t) * n}, {gens_out64, 64 * n}},      // a batch that does not complete shows no item as parsed
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_gen_parse, grid, dim3(256), 0, st, results + i0, gens_out64 + 64 * i0, gens33 + 33 * i0, m);
    });
}
extern "C" int secp256k1_generator_parse_batch(s2k_engine* e, int32_t* results, unsigned char* gens_out64, const unsigned char* gens33, size_t n) {
    const char* who = "secp256k1_generator_parse_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !gens_out64 || !gens33) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n); memset(gens_out64, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, gens_out64, 64 * n}, {gens33, nullptr, 33 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_generator_parse_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), n));
}

// ---- secp256k1_generator_serialize ------------------------------------------------------------------------------------------------
extern "C" int secp256k1_generator_serialize_batch_dev(s2k_engine* e, void* stream, unsigned char* out33, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_generator_serialize_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out33 || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return lanes_run(e, stream, n, {false, false, 0}, {{out33, 33 * n}}, [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_gen_serialize, grid, dim3(256), 0, st, out33 + 33 * i0, gens64 + 64 * i0, m);
    });
}
extern "C" int secp256k1_generator_serialize_batch(s2k_engine* e, unsigned char* out33, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_generator_serialize_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out33 || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(out33, 0, 33 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, out33, 33 * n}, {gens64, nullptr, 64 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_generator_serialize_batch_dev(e, nullptr, b[0].at(), b[1].at(), n));
}

// ---- secp256k1_pedersen_commit ----------------------------------------------------------------------------------------------------
extern "C" int secp256k1_pedersen_commit_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* commits_out33, const unsigned char* blinds32,
                                                   const uint64_t* values, const unsigned char* gens64, size_t n) {
    const char* who = "secp256k1_pedersen_commit_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !commits_out33 || !values || !gens64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}, {commits_out33, 33 * n}},      // a batch that does not complete shows no item as committed
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_pedersen_commit, grid, dim3(256), 0, st, results + i0, commits_out33 + 33 * i0, blinds32 ? blinds32 + 32 * i0 : nullptr, values + i0,
                           gens64 + 64 * i0, e->gtab, e->ptab, m);
    });
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
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, commits_out33, 33 * n}, {blinds32, nullptr, 32 * n}, {values, nullptr, 8 * n}, {gens64, nullptr, 64 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_pedersen_commit_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].opt(), b[3].at<uint64_t>(), b[4].at(), n));
}
