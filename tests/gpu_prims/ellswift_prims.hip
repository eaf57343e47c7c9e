// tests/gpu_prims/ellswift_prims.hip -- TEST-ONLY kernels: the lane routines of ellswift.h run directly on the device, one lane per
// item, where the library's entry points only reach them through the encode loop: the partial inverse for a c the caller chooses, the
// fraction routine's choice of candidate, and the counter / branch helpers.  Whole wavefronts are launched and no lane leaves early
// (the inversion inside the partial inverse is shared by the 64 lanes); a lane without an item reads item 0 and is inactive.  Not part
// of the product library.
#include "../../secp256k1_zkp_amd/csrc/ellswift.h"
#include <hip/hip_runtime.h>

// x32, u32: n * 32 bytes big-endian; c: n ints in 0..7: ok[i], t32 + 32 i = ellswift_xswiftec_inv (t normalised)
__global__ void k_ellswift_inv(int* ok, unsigned char* t32, const unsigned char* x32, const unsigned char* u32_, const int* c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n, ii = live ? i : 0;
    fe x, u, t;
    fe_set_b32_mod(x, x32 + 32 * ii); fe_set_b32_mod(u, u32_ + 32 * ii);
    const int r = ellswift_xswiftec_inv(t, x, u, c[ii], live);
    fe_normalize(t);
    if (live) { ok[i] = r; fe_get_b32(t32 + 32 * i, t); }
}
// which[i] = the candidate ellswift_frac_root takes for ell64 + 64 i (3, 2, 1), with `roots` roots
__global__ void k_ellswift_which(int* which, const unsigned char* ell64, int roots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe u, t, xn, xd, root;
    fe_set_b32_mod(u, ell64 + 64 * i); fe_set_b32_mod(t, ell64 + 64 * i + 32); fe_normalize(t);
    which[i] = ellswift_frac_root(xn, xd, root, u, t, roots);
}
// out[5 i ..] = pool counter, draw counter, byte, shift and branch value of attempt i against the pool hash pool32
__global__ void k_ellswift_schedule(unsigned* out, const unsigned char* pool32, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8], b, s;
    for (int j = 0; j < 8; j++) w[j] = s2k_load_be32(pool32 + 4 * j);
    ellswift_branch_index(b, s, (u32)i);
    out[5 * i] = ellswift_pool_counter((u32)i); out[5 * i + 1] = ellswift_draw_counter((u32)i); out[5 * i + 2] = b; out[5 * i + 3] = s;
    out[5 * i + 4] = (unsigned)ellswift_branch_value(w, (u32)i);
}
// every pointer is device memory holding n items
extern "C" __attribute__((visibility("default")))
int s2k_test_ellswift_inv(int* ok, unsigned char* t32, const unsigned char* x32, const unsigned char* u32_, const int* c, int n) {
    if (n <= 0 || !ok || !t32 || !x32 || !u32_ || !c) return -1;
    hipLaunchKernelGGL(k_ellswift_inv, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, ok, t32, x32, u32_, c, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
extern "C" __attribute__((visibility("default")))
int s2k_test_ellswift_which(int* which, const unsigned char* ell64, int roots, int n) {
    if (n <= 0 || !which || !ell64 || roots < 2 || roots > 3) return -1;
    hipLaunchKernelGGL(k_ellswift_which, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, which, ell64, roots, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
extern "C" __attribute__((visibility("default")))
int s2k_test_ellswift_schedule(unsigned* out, const unsigned char* pool32, int n) {
    if (n <= 0 || !out || !pool32) return -1;
    hipLaunchKernelGGL(k_ellswift_schedule, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, out, pool32, n);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
}
