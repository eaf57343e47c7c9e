// tests/gpu_prims/s2c_prims.hip -- TEST-ONLY kernel: s2c_x_matches (s2c.h), the inversion-free x(R) mod n == r comparison, one item per
// lane on a point the caller chooses.  No entry point of the library reaches x(R) >= n; here the test hands that point in.  Not part of
// the product library.
#include "../../secp256k1_zkp_amd/csrc/s2c.h"
#include <hip/hip_runtime.h>

// xy = affine points (64 bytes, x | y big-endian), z = 32 bytes, r = 32 bytes (< n): out[i] = s2c_x_matches((x z^2, y z^3, z), r)
__global__ void k_s2c_x_matches(int* out, const unsigned char* xy, const unsigned char* z32, const unsigned char* r32, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ge a; fe_set_b32_mod(a.x, xy + 64 * i); fe_set_b32_mod(a.y, xy + 64 * i + 32);
    fe z, z2, z3; fe_set_b32_mod(z, z32 + 32 * i);
    gej R; R.inf = 0;
    fe_sqr(z2, z); fe_mul(z3, z2, z); fe_mul(R.x, a.x, z2); fe_mul(R.y, a.y, z3); R.z = z; fe_norm_weak(R.z);
    scalar r; sc_set_b32(r, r32 + 32 * i, nullptr);
    out[i] = s2c_x_matches(R, r);
}
// every pointer is device memory holding n items
extern "C" __attribute__((visibility("default")))
int s2k_test_s2c_x_matches(int* out, const unsigned char* xy, const unsigned char* z32, const unsigned char* r32, int n) {
    if (n <= 0 || !out || !xy || !z32 || !r32) return -1;
    hipLaunchKernelGGL(k_s2c_x_matches, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, out, xy, z32, r32, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
