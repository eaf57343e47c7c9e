// tests/gpu_prims/ring_six_prims.hip -- TEST-ONLY kernel: the six-base ring form (ecmult.h: ecmult_ring6_tables + ecmult_ring6_step) one
// item per lane, as the rangeproof rings use it: R = e*A + s*G + f*G (the table of G stands in for the generator's).  Not part of the
// product library.
#include "../../secp256k1_zkp_amd/csrc/gtable.h"
#include <hip/hip_runtime.h>

// a = points (64 bytes), b = (e || s || f) 96 bytes per item; flag = 2 * completed + infinity.  One wavefront per 64 items (64-lane
// workgroups).  Three regions of `scratch`, each given by its first word: rtab = n * S2K_RTAB_WORDS, raw = one S2K_RRAW_WAVE_WORDS parking
// area per started wavefront, `raw_stride` words apart (so that the caller can put guard words between them), ptab = n * S2K_PTAB_WORDS
// for the caller's fallback: a wavefront whose step returns 0 (an exceptional addition) takes the general form on the same point, as
// k_rp_rings_shared -> k_rp_rings does.
__global__ void k_ring6(unsigned char* out, int* flag, const unsigned char* a, const unsigned char* b, const u32* gtab, u32* scratch,
                        size_t rtab0, size_t raw0, size_t raw_stride, size_t ptab0, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    __shared__ u32 s_dig[S2K_RING_DIG_WORDS * 256];
    ge p; fe_set_b32_mod(p.x, a + 64 * i); fe_set_b32_mod(p.y, a + 64 * i + 32); fe_norm_weak(p.x); fe_norm_weak(p.y);
    gej A, T1, T2, R; gej_set_ge(A, p);
    T2 = A;
    for (int k = 0; k < 86; k++) {
        if (k == 43) { T1 = T2; fe_norm_weak(T1.y); }
        gej_double_lean(T2, T2);
    }
    fe_norm_weak(T2.y);
    scalar e, sg, f; sc_set_b32(e, b + 96 * i, nullptr); sc_set_b32(sg, b + 96 * i + 32, nullptr); sc_set_b32(f, b + 96 * i + 64, nullptr);
    u32* rtab = scratch + rtab0 + (size_t)i * S2K_RTAB_WORDS;
    u32* raw = scratch + raw0 + (size_t)(i >> 6) * raw_stride + (i & 63);
    u32* ptab = scratch + ptab0 + (size_t)i * S2K_PTAB_WORDS;
    ecmult_ring6_tables(rtab, raw, A, T1, T2);
    const int done = S2K_WAVE_ALL(ecmult_ring6_step(R, rtab, e, sg, f, 1, gtab, gtab, S2K_LANE_DIG(s_dig)));
    if (!done) {
        scalar sf; sc_add(sf, sg, f);
        const lane_mem lm{ptab, S2K_LANE_DIG(s_dig)};
        ecmult_lane(R, A, e, sf, 1, gtab, lm);
    } else R.inf = 0;
    ge r; fe_set_zero(r.x); fe_set_zero(r.y);
    if (!R.inf) ge_set_gej(r, R);
    flag[i] = 2 * done + (R.inf ? 1 : 0);
    fe_normalize(r.x); fe_normalize(r.y); fe_get_b32(out + 64 * i, r.x); fe_get_b32(out + 64 * i + 32, r.y);
}
// scratch_words: the size of `scratch`; refuses (returns -1, launches nothing) a region that does not lie inside it
extern "C" __attribute__((visibility("default")))
int s2k_test_ring6(unsigned char* out, int* flag, const unsigned char* a, const unsigned char* b, const void* gtab, unsigned* scratch, size_t scratch_words,
                   size_t rtab0, size_t raw0, size_t raw_stride, size_t ptab0, int n) {
    if (n <= 0 || raw_stride < S2K_RRAW_WAVE_WORDS) return -1;
    const size_t waves = ((size_t)n + 63) / 64;
    if (rtab0 + (size_t)n * S2K_RTAB_WORDS > scratch_words || raw0 + (waves - 1) * raw_stride + S2K_RRAW_WAVE_WORDS > scratch_words || ptab0 + (size_t)n * S2K_PTAB_WORDS > scratch_words) return -1;
    hipLaunchKernelGGL(k_ring6, dim3((unsigned)waves), dim3(64), 0, 0, out, flag, a, b, (const u32*)gtab, (u32*)scratch, rtab0, raw0, raw_stride, ptab0, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
extern "C" __attribute__((visibility("default")))
int s2k_test_ring6_sizes(int* out4) { out4[0] = S2K_RTAB_WORDS; out4[1] = S2K_RRAW_WAVE_WORDS; out4[2] = S2K_PTAB_WORDS; out4[3] = S2K_R6_PARK_WORDS; return 4; }
