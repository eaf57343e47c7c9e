// tests/gpu_prims/ring_step_trim_prims.hip -- TEST-ONLY kernel: the signed-accumulator forms of the six-base ring step (group.h:
// gej_dblneg_ring, gej_rsub_ge_ring, gez_add_ge_ring) one item per lane on coordinates given as raw limbs, for a limb-for-limb comparison
// with the host emulation (tests/host_emul/ring_step_trim_emu.cpp runs the same wrappers).  Not part of the product library.
#include "../../secp256k1_zkp_amd/csrc/gtable.h"
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "ring_step_trim_forms.h"

// kind 0: doubling, x = +X (in 27 words, out 27); 1: doubling, x = -X; 2: operand - point (in 45, out 27 + the same-x flag);
// 3: the XYZZ addition (in 54, out 36).  Item i reads in[i * in_words ..] and writes out[i * 37 ..] (word 36 = flag).
#define TRIM_OUT_WORDS 37
__global__ void k_trim_forms(u32* out, const u32* in, int kind, int in_words, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* p = in + (size_t)i * in_words;
    u32* o = out + (size_t)i * TRIM_OUT_WORDS;
    if (kind <= 2) {
        gej a, r; trim_load(a.x, p); trim_load(a.y, p + 9); trim_load(a.z, p + 18); a.inf = 0;
        int flag = 0;
        if (kind == 2) { ge b; trim_load(b.x, p + 27); trim_load(b.y, p + 36); flag = trim_rsub(r, a, b); }
        else trim_dbl(r, a, kind);
        trim_store(o, r.x); trim_store(o + 9, r.y); trim_store(o + 18, r.z);
        o[36] = (u32)flag;
    } else {
        gez a; ge b; trim_load(a.x, p); trim_load(a.y, p + 9); trim_load(a.zz, p + 18); trim_load(a.zzz, p + 27); a.inf = 0; trim_load(b.x, p + 36); trim_load(b.y, p + 45);
        trim_gez(a, b);
        trim_store(o, a.x); trim_store(o + 9, a.y); trim_store(o + 18, a.zz); trim_store(o + 27, a.zzz);
        o[36] = 0;
    }
}
// in_have / out_have: the sizes of the two buffers in words; refuses (returns -1, launches nothing) what does not fit them
extern "C" __attribute__((visibility("default")))
int s2k_test_trim_forms(unsigned* out, size_t out_have, const unsigned* in, size_t in_have, int kind, int n) {
    if (n <= 0 || kind < 0 || kind > 3) return -1;
    const int in_words = kind <= 1 ? 27 : kind == 2 ? 45 : 54;
    if ((size_t)n * in_words > in_have || (size_t)n * TRIM_OUT_WORDS > out_have) return -1;
    (void)hipGetLastError();                        // what an earlier call of the process left behind is not this launch's
    hipLaunchKernelGGL(k_trim_forms, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (u32*)out, (const u32*)in, kind, in_words, n);
    const hipError_t launched = hipGetLastError(), done = hipDeviceSynchronize();
    if (launched != hipSuccess || done != hipSuccess) fprintf(stderr, "s2k_test_trim_forms: launch: %s, synchronize: %s\n", hipGetErrorString(launched), hipGetErrorString(done));
    return launched == hipSuccess && done == hipSuccess;
}
