// tests/wave_inverse/waveinv_lanes_test.hip -- TEST-ONLY kernels for the uniform inverse of csrc/modinv.h: the lane-distributed form
// (ds_inverse_words_lanes) next to the scalar-apply form (ds_inverse_words<true>), for both moduli, the lane form's state after
// every batch, and its carry step (dsl_carry) alone on column sums handed in per lane.  One value per wavefront, the same in all its
// 64 lanes.  For tests/test_gpu_wave_inverse_lanes.py; not part of the product library.
#include "../../secp256k1_zkp_amd/csrc/modinv.h"
#include <hip/hip_runtime.h>

#define WL_DUMP_WORDS (4 * DS_LIMBS * DS_BATCHES)

// form 0: lanes, 1: scalar apply, 2: lanes with the state dump.  in: 8 words per wavefront; out: 8 words per LANE (every lane of a
// wavefront must hold the same result); dump: WL_DUMP_WORDS per wavefront, batches: one count per wavefront (form 2 only).
template <int MOD>
__global__ void k_uniform_inverse(int form, u32* out, int32_t* dump, int* batches, const u32* in, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((i & ~63) >= n) return;                 // whole wavefronts only: n is a multiple of 64
    const int wv = i >> 6;
    const ds_modulus md = MOD ? DS_MOD_N : DS_MOD_P;
    u32 w[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (u32)__builtin_amdgcn_readfirstlane((int)in[(size_t)8 * wv + k]);
    if (form == 0) ds_inverse_words_lanes(o, w, md);
    else if (form == 1) ds_inverse_words<true>(o, w, md);
    else {
        int nb = 0;
        ds_inverse_words_lanes<true>(o, w, md, dump + (size_t)WL_DUMP_WORDS * wv, &nb);
        if ((i & 63) == 0) batches[wv] = nb;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[(size_t)8 * i + k] = o[k];
}

extern "C" int s2k_test_uniform_inverse(int form, int mod, u32* out, int32_t* dump, int* batches, const u32* in, int n, int block) {
    if (n % 64 != 0 || block % 64 != 0 || block <= 0 || block > 1024 || form < 0 || form > 2) return 0;
    if (form == 2 && (!dump || !batches)) return 0;
    const dim3 grid((n + block - 1) / block), blk(block);
    if (mod) hipLaunchKernelGGL(k_uniform_inverse<1>, grid, blk, 0, 0, form, out, dump, batches, in, n);
    else hipLaunchKernelGGL(k_uniform_inverse<0>, grid, blk, 0, 0, form, out, dump, batches, in, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}

// dsl_carry on its own: lane l of every wavefront takes the column sum s[i] (lanes 0..8 of a wavefront are meaningful, the others hold 0) and
// writes the limb that comes out, with the lane masks ds_inverse_words_lanes uses.
__global__ void k_lane_carry(int32_t* out, const int64_t* s, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((i & ~63) >= n) return;
    const u32 lane = (u32)(threadIdx.x & 63u);
    const int32_t lm = lane < DS_LIMBS - 1 ? DS_MASK : -1, cm = lane < DS_LIMBS - 1 ? -1 : 0;
    out[i] = dsl_carry(s[i], lm, cm);
}

extern "C" int s2k_test_lane_carry(int32_t* out, const int64_t* s, int n, int block) {
    if (n % 64 != 0 || block % 64 != 0 || block <= 0 || block > 1024) return 0;
    hipLaunchKernelGGL(k_lane_carry, dim3((n + block - 1) / block), dim3(block), 0, 0, out, s, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
