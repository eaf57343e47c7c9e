// Micro-benchmark: what one to-affine inversion costs a VALU-bound kernel -- per-lane fe_inv (modinv.h) against the wave-batched
// fe_inv_wave (waveinv.h), whose division-step control runs on the scalar unit, in its two forms.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../secp256k1_zkp_amd/csrc -o waveinv_bench waveinv_bench.hip
//   ./waveinv_bench [iters] [VALU per fe_mul pair] [F]
// Three forms in one run: per-lane fe_inv, fe_inv_wave with the matrix application on the scalar unit (fe_inv_wave<true>, the earlier
// form), and fe_inv_wave with it across the lanes (fe_inv_wave<false>, modinv.h: ds_inverse_words_lanes).
// Every wavefront runs `iters` rounds of { F dependent fe_mul pairs (the VALU-bound filler: point arithmetic) ; one inversion }, at
// exactly 2 waves per SIMD (256-lane workgroups holding 80 KiB of LDS each: two per CU), the occupancy of k_rp_rings_shared.  The waves
// drift apart, so one wave's inversion runs beside the other's filler as in the kernel.  The cost of an inversion is the time it adds
// to a round, expressed in filler VALU instructions: (t_inv - t_filler) / t_filler * (filler VALU per round).  The filler's VALU count
// per fe_mul pair is taken from the compiled code (tools/static_count/loops.py on this file's -S output: 314).  F sets how much of a
// round the inversion is: with F = 24 two waves of a SIMD are mostly inverting at the same time; a ring position of k_rp_rings_shared is
// ~250 000 VALU instructions around one inversion, F ~ 800.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "waveinv.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

extern __shared__ unsigned char dyn_lds[];

template <int MODE>                             // 0: filler only, 1: + fe_inv per lane, 2: + fe_inv_wave, scalar apply, 3: + fe_inv_wave, lanes
__global__ void __launch_bounds__(256, 2) k_round(u32* out, u32 seed, int iters, int filler) {
    if (seed == 0xdeadbeefu) dyn_lds[threadIdx.x] = 1;
    fe a, b, c, d;
    const u32 t = threadIdx.x + blockIdx.x * 256u + seed;
#pragma unroll
    for (int i = 0; i < FE_LIMBS; i++) {
        a.n[i] = (t * 2654435761u + 17u * i) & (i == 8 ? FE_TOPM : FE_M);
        b.n[i] = (t * 40503u + 29u * i + 1u) & (i == 8 ? FE_TOPM : FE_M);
        c.n[i] = a.n[i] ^ 0x55u; d.n[i] = b.n[i] ^ 0x33u;
    }
    int okall = 1;
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
#pragma unroll 1
        for (int k = 0; k < filler; k++) fe_mul2(a, a, b, c, c, d);
        if (MODE == 1) { fe r; fe_inv(r, a); b = r; }
        if (MODE == 2) { fe r; okall &= fe_inv_wave<true>(r, a); b = r; }
        if (MODE == 3) { fe r; okall &= fe_inv_wave<false>(r, a); b = r; }
    }
    u32 x = (u32)okall;
#pragma unroll
    for (int i = 0; i < FE_LIMBS; i++) x ^= a.n[i] ^ c.n[i] ^ b.n[i];
    out[blockIdx.x * 256u + threadIdx.x] = x;
}

template <int MODE>
static double run(int blocks, int iters, int filler, u32* out) {
    const size_t lds = 80 * 1024;
    CHECK(hipFuncSetAttribute((const void*)k_round<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_round<MODE>, dim3(blocks), dim3(256), lds, 0, out, 1u, 2, filler);          // warm-up
    CHECK(hipDeviceSynchronize());
    double best = 1e30;
    for (int rep = 0; rep < 5; rep++) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_round<MODE>, dim3(blocks), dim3(256), lds, 0, out, 1u, iters, filler);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    CHECK(hipGetLastError());
    return best;
}

int main(int argc, char** argv) {
    hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
    const int blocks = 2 * prop.multiProcessorCount;        // two 256-lane workgroups per CU = two waves per SIMD
    const int iters = argc > 1 ? atoi(argv[1]) : 200;
    const double filler_valu = argc > 2 ? atof(argv[2]) : 0.0;     // VALU per fe_mul pair (from the static count), 0: report fe_mul-pair units
    const int filler = argc > 3 ? atoi(argv[3]) : 24;
    u32* out; CHECK(hipMalloc(&out, (size_t)blocks * 256 * sizeof(u32)));
    const double t0 = run<0>(blocks, iters, filler, out), t1 = run<1>(blocks, iters, filler, out), t2 = run<2>(blocks, iters, filler, out), t3 = run<3>(blocks, iters, filler, out);
    const double c1 = (t1 - t0) / t0 * filler, c2 = (t2 - t0) / t0 * filler, c3 = (t3 - t0) / t0 * filler;       // in fe_mul pairs of the filler
    printf("{\"cus\": %d, \"blocks\": %d, \"iters\": %d, \"filler_pairs\": %d, \"ms_filler\": %.4f, \"ms_fe_inv\": %.4f, \"ms_fe_inv_wave_scalar\": %.4f, \"ms_fe_inv_wave_lanes\": %.4f,\n",
           prop.multiProcessorCount, blocks, iters, filler, t0, t1, t2, t3);
    printf(" \"cost_fe_inv_pairs\": %.2f, \"cost_wave_scalar_pairs\": %.2f, \"cost_wave_lanes_pairs\": %.2f, \"wave_scalar_over_lane\": %.4f, \"wave_lanes_over_lane\": %.4f",
           c1, c2, c3, c2 / c1, c3 / c1);
    if (filler_valu > 0) printf(", \"cost_fe_inv_valu_eq\": %.0f, \"cost_wave_scalar_valu_eq\": %.0f, \"cost_wave_lanes_valu_eq\": %.0f", c1 * filler_valu, c2 * filler_valu, c3 * filler_valu);
    printf("}\n");
    CHECK(hipFree(out));
    return 0;
}
