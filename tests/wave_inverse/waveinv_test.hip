// tests/wave_inverse/waveinv_test.hip -- TEST-ONLY kernels for csrc/waveinv.h: the wave-batched inverse (fe_inv_wave) next to the per-lane
// fe_inv and fe_inv_fermat, on the same raw 9-limb inputs, so that tests/test_gpu_wave_inverse.py can compare the three with each
// other and with Python.  Not part of the product library.
#include "../../secp256k1_zkp_amd/csrc/waveinv.h"
#include <hip/hip_runtime.h>

// op 0: fe_inv_wave (flag = its return value), 1: fe_inv, 2: fe_inv_fermat.  in: 9 raw limbs per lane; out: 8 canonical words per lane.
__global__ void k_waveinv(int op, u32* out, int* flag, const u32* in, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((i & ~63) >= n) return;                 // whole wavefronts only: n is a multiple of 64
    fe z, r;
#pragma unroll
    for (int k = 0; k < FE_LIMBS; k++) z.n[k] = in[(size_t)FE_LIMBS * i + k];
    int ok = 1;
    if (op == 0) ok = fe_inv_wave(r, z);
    else if (op == 1) fe_inv(r, z);
    else fe_inv_fermat(r, z);
    fe_normalize(r);
    u32 w[8]; fe_to_words(w, r);
#pragma unroll
    for (int k = 0; k < 8; k++) out[(size_t)8 * i + k] = w[k];
    flag[i] = ok;
}

extern "C" int s2k_test_waveinv(int op, u32* out, int* flag, const u32* in, int n, int block) {
    if (n % 64 != 0 || block % 64 != 0 || block <= 0 || block > 1024) return 0;
    hipLaunchKernelGGL(k_waveinv, dim3((n + block - 1) / block), dim3(block), 0, 0, op, out, flag, in, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
