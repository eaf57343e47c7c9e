// engine_verdict.h -- what the verifiers that answer a whole batch with ONE verdict share: a hash tree over the item digests gives the seed
// of the random coefficients, one multi-scalar multiplication gives a point, and the verdict is "nothing was refused and the point is
// infinity".  engine_schnorr_all.hip and engine_bppp_all.hip use all of it, engine_halfagg.hip the final kernel.  The kernels are static
// templates: every unit that includes this file gets its own copy (no -fgpu-rdc), and only of those it launches.
#pragma once
#include "engine_lanes.h"
#include "schnorr_all.h"

template <int = 0>
static __global__ void __launch_bounds__(256)
k_verdict_node(u32* out, const u32* __restrict__ in, sa_midstates mid, size_t cnt_in, size_t cnt_out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt_out) return;
    const size_t left = cnt_in - SA_FANIN * j;
    sa_node(out + 8 * j, mid, in + 8 * SA_FANIN * j, left < SA_FANIN ? (u32)left : SA_FANIN);
}
template <int = 0>
static __global__ void k_verdict_final(int32_t* verdict, const u32* flags, const u32* res28) {
    if (threadIdx.x || blockIdx.x) return;
    *verdict = (flags[0] == 0u) && (res28[27] != 0u);
}
// the levels above the n item digests at `nodes` (sa_node_count(n) records of 8 words, level after level); returns the root
// (a template like its kernel: a unit that grows no tree gets neither)
template <int = 0>
static const u32* verdict_tree(hipStream_t st, u32* nodes, const sa_midstates& mid, size_t n) {
    size_t counts[SA_MAX_LEVELS];
    const int levels = sa_level_plan(counts, n);
    u32* level = nodes;
    for (int k = 0; k + 1 < levels; k++) {
        u32* next = level + 8 * counts[k];
        hipLaunchKernelGGL(k_verdict_node<>, dim3((unsigned)((counts[k + 1] + 255) / 256)), dim3(256), 0, st, next, (const u32*)level, mid, counts[k], counts[k + 1]);
        level = next;
    }
    return level;
}
// A family's four events (created at its first call): [0],[1] its own phase boundaries, [2],[3] stand-ins.  msm_launch records ev[2] / ev[3]
// around its own dominant kernel: for the duration of that call the two slots hold the stand-ins (the engine's lock is held), so that
// ev[2] .. ev[3] -- s2k_engine_last_ms(1) -- is the whole MSM.
static int verdict_events(hipEvent_t (&ev4)[4]) {
    for (int k = 0; k < 4; k++) if (!ev4[k]) HIPCHK(hipEventCreate(&ev4[k]));
    return 1;
}
// the end of a launch: ev[2], the MSM over n_pts points and the generator term, ev[3], the verdict, ev[1]
static int verdict_tail(s2k_engine* e, hipStream_t st, ws_carver& c, hipEvent_t (&ev4)[4], int32_t* d_verdict, const u32* d_flags, const unsigned char* d_gsc,
                        const unsigned char* d_sc, const unsigned char* d_pts, const unsigned char* d_inf, size_t n_pts) {
    HIPCHK(hipEventRecord(e->ev[2], st));
    u32* res28 = nullptr;
    hipEvent_t const keep2 = e->ev[2], keep3 = e->ev[3];
    e->ev[2] = ev4[2]; e->ev[3] = ev4[3];
    const int ok = msm_launch(e, st, c, &res28, d_gsc, d_sc, d_pts, d_inf, n_pts);
    e->ev[2] = keep2; e->ev[3] = keep3;
    if (!ok) return 0;
    HIPCHK(hipEventRecord(e->ev[3], st));
    hipLaunchKernelGGL(k_verdict_final<>, dim3(1), dim3(64), 0, st, d_verdict, d_flags, (const u32*)res28);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
// the `_dev` reply for a batch with nothing to launch: the verdict word, and the seed 32 zero bytes
static int verdict_reply(hipStream_t st, int32_t* verdict_dev, unsigned char* seed32_out_dev, u32 verdict) {
    launch_set_word(st, (u32*)verdict_dev, verdict);
    HIPCHK(hipGetLastError());
    if (seed32_out_dev) HIPCHK(hipMemsetAsync(seed32_out_dev, 0, 32, st));
    return 1;
}
// the four phases of the family's most recent call, in ms, once its work is complete (s2k_engine_sync); -1 where no such call has run
static int verdict_split_ms(const char* who, s2k_engine* e, hipEvent_t (s2k_engine::*family)[4], float* out4) {
    if (!e) return s2k_fail(who, "null engine");
    if (!out4) return s2k_fail_arg(who, "illegal argument");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    hipEvent_t (&ev4)[4] = e->*family;
    for (int k = 0; k < 4; k++) out4[k] = -1.0f;
    if (!ev4[0] || !ev4[1]) return 1;
    hipEvent_t const b[5] = {e->ev[0], ev4[0], ev4[1], e->ev[2], e->ev[3]};
    for (int k = 0; k < 4; k++) if (hipEventElapsedTime(&out4[k], b[k], b[k + 1]) != hipSuccess) { (void)hipGetLastError(); out4[k] = -1.0f; }
    return 1;
}
// The host form: the family's inputs `in`, uploaded behind `front` bytes (the locating call carves the workspace from offset 0 again, and
// must neither grow it nor overwrite the uploads: front covers the larger of the two device parts), then the scratch of the locating
// call's results, the seed and the verdict.  launch(st, c, d_verdict, d_seed, b) is the family's launch with its carver at 0 and b[i] the
// staged in[i]; where the verdict is 0 and the caller wants results, locate(d_res, b) runs the per-item verifier on the engine's stream
// over the buffers already uploaded.
template <size_t N, class Launch, class Locate>
static int verdict_host(s2k_engine* e, const stage_buf (&in)[N], size_t front, int32_t* verdict, int32_t* results, unsigned char* seed32_out, size_t n, Launch launch,
                        Locate locate) {
    stage_buf b[N + 3];
    std::copy(in, in + N, b);
    b[N] = stage_buf{nullptr, nullptr, 4 * n, 64}; b[N + 1] = stage_buf{nullptr, seed32_out, 32, 32}; b[N + 2] = stage_buf{nullptr, verdict, 4, 12};
    hipStream_t st = e->stream;
    {
        if (!stage_open(e, b, front)) return 0;
        stream_guard sg(e, st);
        ws_carver c{e->ws, 0};
        if (!stage_close(e, b, launch(st, c, (int32_t*)b[N + 2].dev, seed32_out ? b[N + 1].dev : nullptr, (const stage_buf*)b))) return 0;
    }
    if (!results) return 1;
    if (*verdict) { for (size_t i = 0; i < n; i++) results[i] = 1; return 1; }
    if (!locate((int32_t*)b[N].dev, (const stage_buf*)b)) return 0;
    HIPCHK(hipMemcpyAsync(results, b[N].dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 1;
}
