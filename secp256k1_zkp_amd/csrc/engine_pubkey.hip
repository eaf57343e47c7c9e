#include "engine_lanes.h"
#include "pubkey.h"

// ------------------------------------------------------------------------------------------------------------
// Public keys (pubkey.h): conversion between the five encodings, negation, tweak-mul, combine
// ------------------------------------------------------------------------------------------------------------
// Convert / negate and tweak-mul are one item per lane behind lanes_run.  Combine is a launch chain on the caller's stream, planned on
// the host from the set offsets with musig_agg.h's plan (musig_agg_plan_sum at this family's fan-in F): pass 0 is this unit's kernel
// (one lane per chunk of up to F consecutive keys of one set, folded from the key bytes), passes 1 .. are the segmented sum of
// engine_musig_agg.hip, reached through its host function agg_sum_launch (engine_internal.h), and the finish is one set per lane.  A
// batch whose sets all fit one chunk has a one-pass plan: two launches.
// The fused pass 0 serves the formats whose load is cheap (1, 3, 4).  Keys in formats 0 and 2 cost a square root each, and F roots
// one after the other in one lane leave the machine idle where one root per lane fills it, so those take the load-then-fold chain: one
// key per lane to a partial (k_pubkey_partial), then every pass through agg_sum_launch (DESIGN.md 7.10 has both measured against each
// other).  -DS2K_PK_FOLD_FUSED=0 builds the load-then-fold chain for every format: the control of that A/B.
#ifndef S2K_PK_FOLD_FUSED
#define S2K_PK_FOLD_FUSED 1
#endif

// (no lane leaves early in k_pubkey_tweak_mul and k_pubkey_combine_finish: ecmult_lane builds its tables in lock step and the to-affine
// inversion is shared by the 64 lanes of a wavefront)
__global__ void __launch_bounds__(256)
k_pubkey_convert(int32_t* __restrict__ results, unsigned char* __restrict__ out, int out_format, unsigned char* __restrict__ parities, const unsigned char* __restrict__ in,
                 int in_format, int negate, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    results[i] = pubkey_convert_lane(out + pubkey_bytes(out_format) * i, out_format, parities ? parities + i : nullptr, in + pubkey_bytes(in_format) * i, in_format, negate, 1);
}
__global__ void __launch_bounds__(256, 2)
k_pubkey_tweak_mul(int32_t* __restrict__ results, unsigned char* __restrict__ out, int out_format, unsigned char* __restrict__ parities, const unsigned char* __restrict__ keys,
                   int key_format, const unsigned char* __restrict__ tweaks32, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t n) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < n;
    const size_t i = live ? lane : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + lane * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = pubkey_tweak_mul_lane(out + pubkey_bytes(out_format) * i, out_format, parities ? parities + i : nullptr, keys + pubkey_bytes(key_format) * i, key_format,
                                        tweaks32 + 32 * i, live, gtab, lm);
    if (live) results[i] = r;
}
// combine, pass 0: outputs [j0, j0 + m) of the plan's first pass
__global__ void __launch_bounds__(256)
k_pubkey_fold(u32* __restrict__ out, int32_t* __restrict__ flag, const unsigned char* __restrict__ keys, int key_format, const u64* __restrict__ in_off,
              const u64* __restrict__ out_off, size_t nseg, unsigned fanin, size_t j0, size_t m) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= m) return;
    flag[j0 + lane] = pubkey_fold_item(out, keys, key_format, in_off, out_off, nseg, fanin, j0 + lane);
}
// (the load-then-fold chain's pass in front of the fold: one key per lane)
__global__ void __launch_bounds__(256)
k_pubkey_partial(u32* __restrict__ out, int32_t* __restrict__ flag, const unsigned char* __restrict__ keys, int key_format, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = pubkey_partial_lane(out + (size_t)MUSIG_AGG_GEJ_WORDS * i, keys + pubkey_bytes(key_format) * i, key_format);
}
// combine, finish: set k's flags are flag[flag_off[k] .. flag_off[k + 1])
__global__ void __launch_bounds__(256)
k_pubkey_combine_finish(int32_t* __restrict__ results, unsigned char* __restrict__ out, int out_format, unsigned char* __restrict__ parities, const u32* __restrict__ sums,
                        const int32_t* __restrict__ flag, const u64* __restrict__ key_off, const u64* __restrict__ flag_off, size_t n_sets) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < n_sets;
    const size_t k = live ? lane : 0;
    const u64 m = live ? key_off[k + 1] - key_off[k] : 0, first = flag_off[k], count = live ? flag_off[k + 1] - first : 0;
    const int r = pubkey_combine_finish_lane(out + pubkey_bytes(out_format) * k, out_format, parities ? parities + k : nullptr, sums + (size_t)MUSIG_AGG_GEJ_WORDS * k, flag,
                                             first, count, m, live);
    if (live) results[k] = r;
}

static int pubkey_formats_ok(const char* who, int out_format, int in_format) {
    if (!pubkey_out_format_ok(out_format)) return s2k_fail_arg(who, "out_format must be S2K_PK_XONLY .. S2K_PK_XONLY_OBJECT (0 .. 5)");
    if (!pubkey_in_format_ok(in_format)) return s2k_fail_arg(who, "the input format must be S2K_PK_XONLY .. S2K_PK_AFFINE (0 .. 4)");
    return 1;
}

// ---- convert and negate ------------------------------------------------------------------------------------------------------------------
static int convert_dev(const char* who, s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                       const unsigned char* in, int in_format, int negate, size_t n) {
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !out || !in) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!pubkey_formats_ok(who, out_format, in_format)) return 0;
    const size_t ob = pubkey_bytes(out_format), ib = pubkey_bytes(in_format);
    auto launch = [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_pubkey_convert, grid, dim3(256), 0, st, results + i0, out + ob * i0, out_format, parities_out ? parities_out + i0 : nullptr, in + ib * i0, in_format,
                           negate, m);
    };
    if (!parities_out) return lanes_run(e, stream, n, {false, false, 0}, {{results, sizeof(int32_t) * n}, {out, ob * n}}, launch);
    return lanes_run(e, stream, n, {false, false, 0}, {{results, sizeof(int32_t) * n}, {out, ob * n}, {parities_out, n}}, launch);
}
static int convert_host(const char* who, s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* in,
                        int in_format, int negate, size_t n) {
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !out || !in) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (parities_out) memset(parities_out, 0, n);
    if (pubkey_out_format_ok(out_format)) memset(out, 0, pubkey_bytes(out_format) * n);
    if (!pubkey_formats_ok(who, out_format, in_format)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, out, pubkey_bytes(out_format) * n}, {nullptr, parities_out, n}, {in, nullptr, pubkey_bytes(in_format) * n, 64}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, convert_dev(who, e, nullptr, b[0].at<int32_t>(), b[1].at(), out_format, parities_out ? b[2].at() : nullptr, b[3].at(), in_format, negate, n));
}
extern "C" int secp256k1_ec_pubkey_convert_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                     const unsigned char* in, int in_format, size_t n) {
    return convert_dev("secp256k1_ec_pubkey_convert_batch_dev", e, stream, results, out, out_format, parities_out, in, in_format, 0, n);
}
extern "C" int secp256k1_ec_pubkey_convert_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* in,
                                                 int in_format, size_t n) {
    return convert_host("secp256k1_ec_pubkey_convert_batch", e, results, out, out_format, parities_out, in, in_format, 0, n);
}
extern "C" int secp256k1_ec_pubkey_negate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                    const unsigned char* in, int in_format, size_t n) {
    return convert_dev("secp256k1_ec_pubkey_negate_batch_dev", e, stream, results, out, out_format, parities_out, in, in_format, 1, n);
}
extern "C" int secp256k1_ec_pubkey_negate_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* in,
                                                int in_format, size_t n) {
    return convert_host("secp256k1_ec_pubkey_negate_batch", e, results, out, out_format, parities_out, in, in_format, 1, n);
}

// ---- tweak-mul ----------------------------------------------------------------------------------------------------------------------------
extern "C" int secp256k1_ec_pubkey_tweak_mul_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                       const unsigned char* keys, int key_format, const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_ec_pubkey_tweak_mul_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !out || !keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!pubkey_formats_ok(who, out_format, key_format)) return 0;
    const size_t ob = pubkey_bytes(out_format), kb = pubkey_bytes(key_format);
    auto launch = [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_pubkey_tweak_mul, grid, dim3(256), 0, st, results + i0, out + ob * i0, out_format, parities_out ? parities_out + i0 : nullptr, keys + kb * i0,
                           key_format, tweaks32 + 32 * i0, e->gtab, e->ptab, m);
    };
    if (!parities_out) return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}, {out, ob * n}}, launch);
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}, {out, ob * n}, {parities_out, n}}, launch);
}
extern "C" int secp256k1_ec_pubkey_tweak_mul_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* keys,
                                                   int key_format, const unsigned char* tweaks32, size_t n) {
    const char* who = "secp256k1_ec_pubkey_tweak_mul_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !out || !keys || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (parities_out) memset(parities_out, 0, n);
    if (pubkey_out_format_ok(out_format)) memset(out, 0, pubkey_bytes(out_format) * n);
    if (!pubkey_formats_ok(who, out_format, key_format)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, results, 4 * n}, {nullptr, out, pubkey_bytes(out_format) * n}, {nullptr, parities_out, n}, {keys, nullptr, pubkey_bytes(key_format) * n, 64},
                     {tweaks32, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ec_pubkey_tweak_mul_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), out_format, parities_out ? b[2].at() : nullptr, b[3].at(),
                                                                     key_format, b[4].at(), n));
}

// ---- combine ------------------------------------------------------------------------------------------------------------------------------
typedef musig_agg_sum_plan agg_sum_plan;
static unsigned fold_fanin(const s2k_engine* e) { return e->pubkey_fold_fanin ? (unsigned)e->pubkey_fold_fanin : (unsigned)PUBKEY_FOLD_FANIN_DEFAULT; }
static int combine_fused(int key_format) { return S2K_PK_FOLD_FUSED && key_format != S2K_PK_XONLY && key_format != S2K_PK_COMPRESSED; }
// the most partials an array of the chain holds: from array 1 on in the fused form (array 0 is the key bytes themselves)
static size_t combine_cap(const agg_sum_plan& p, int fused) {
    if (!fused) return p.cap;
    size_t cap = 0;
    for (size_t q = 1; q <= p.passes; q++) cap = std::max(cap, (size_t)p.offs[q * (p.nseg + 1) + p.nseg]);
    return cap;
}
// flags: one per output of pass 0 (fused), one per key (load-then-fold)
static size_t combine_flags(const agg_sum_plan& p, int fused) { return (size_t)p.offs[(fused ? 1 : 0) * (p.nseg + 1) + p.nseg]; }
static size_t combine_ws(const agg_sum_plan& p, int fused) {
    const size_t part = (size_t)4 * MUSIG_AGG_GEJ_WORDS * combine_cap(p, fused);
    return ws_need({8 * p.offs.size(), part, part, 4 * combine_flags(p, fused)});
}
// every array on the device; the carver continues behind whatever the caller staged.  The offset arrays reach the workspace from
// PAGEABLE host memory (the plan's vector, never the caller's array), as in engine_musig_agg.hip: staged before hipMemcpyAsync returns.
static int combine_run(s2k_engine* e, hipStream_t st, ws_carver& w, const agg_sum_plan& p, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                       const unsigned char* keys, int key_format, size_t n_sets) {
    const unsigned fanin = fold_fanin(e);
    const int fused = combine_fused(key_format);
    const size_t cap = combine_cap(p, fused), n_flags = combine_flags(p, fused);
    agg_sum_bufs s; s.d_off = w.take<u64>(p.offs.size()); s.a = w.take<u32>((size_t)MUSIG_AGG_GEJ_WORDS * cap); s.b = w.take<u32>((size_t)MUSIG_AGG_GEJ_WORDS * cap);
    int32_t* flag = w.take<int32_t>(n_flags);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n_sets, st));
    HIPCHK(hipMemsetAsync(out, 0, pubkey_bytes(out_format) * n_sets, st));
    if (parities_out) HIPCHK(hipMemsetAsync(parities_out, 0, n_sets, st));
    HIPCHK(hipMemcpyAsync(s.d_off, p.offs.data(), 8 * p.offs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    const u32* sums = nullptr;
    const u64* flag_off = s.d_off;
    if (fused) {
        const u64* in_off = s.d_off; const u64* out_off = s.d_off + n_sets + 1;
        for (size_t j0 = 0; j0 < n_flags; j0 += e->max_lanes) {             // pass 0 writes s.b: what pass 1 reads
            const size_t m = std::min(n_flags - j0, e->max_lanes);
            hipLaunchKernelGGL(k_pubkey_fold, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, s.b, flag, keys, key_format, in_off, out_off, n_sets, fanin, j0, m);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev[3], st));
        if (!agg_sum_launch(e, st, p, s, fanin, &sums, 1)) return 0;
        flag_off = out_off;
    } else {
        if (n_flags) hipLaunchKernelGGL(k_pubkey_partial, dim3((unsigned)((n_flags + 255) / 256)), dim3(256), 0, st, s.a, flag, keys, key_format, n_flags);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev[3], st));
        if (!agg_sum_launch(e, st, p, s, fanin, &sums, 0)) return 0;
    }
    hipLaunchKernelGGL(k_pubkey_combine_finish, dim3((unsigned)((n_sets + 255) / 256)), dim3(256), 0, st, results, out, out_format, parities_out, sums, (const int32_t*)flag,
                       (const u64*)s.d_off, flag_off, n_sets);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
// what the entry points check behind their NULL checks of results, out and offsets (the host form zeroes its outputs in between)
static int combine_args(const char* who, int out_format, const unsigned char* keys, int key_format, const uint64_t* key_off, size_t n_sets) {
    if (key_off[n_sets] && !keys) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!pubkey_formats_ok(who, out_format, key_format)) return 0;
    if (key_off[0] != 0) return s2k_fail_arg(who, "offsets must start at 0");
    for (size_t k = 0; k < n_sets; k++) if (key_off[k + 1] < key_off[k]) return s2k_fail_arg(who, "offsets must not decrease");
    return 1;
}
extern "C" int secp256k1_ec_pubkey_combine_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out,
                                                     const unsigned char* keys, int key_format, const uint64_t* key_off, size_t n_sets) {
    const char* who = "secp256k1_ec_pubkey_combine_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sets == 0) return 1;
    if (!results || !out || !key_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!combine_args(who, out_format, keys, key_format, key_off, n_sets)) return 0;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const agg_sum_plan p = musig_agg_plan_sum(key_off, n_sets, fold_fanin(e));
    if (!engine_workspace(e, combine_ws(p, combine_fused(key_format)))) return 0;
    ws_carver w{e->ws, 0};
    return combine_run(e, st, w, p, results, out, out_format, parities_out, keys, key_format, n_sets);
}
extern "C" int secp256k1_ec_pubkey_combine_batch(s2k_engine* e, int32_t* results, unsigned char* out, int out_format, unsigned char* parities_out, const unsigned char* keys,
                                                 int key_format, const uint64_t* key_off, size_t n_sets) {
    const char* who = "secp256k1_ec_pubkey_combine_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sets == 0) return 1;
    if (!results || !out || !key_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n_sets);
    if (parities_out) memset(parities_out, 0, n_sets);
    if (pubkey_out_format_ok(out_format)) memset(out, 0, pubkey_bytes(out_format) * n_sets);
    if (!combine_args(who, out_format, keys, key_format, key_off, n_sets)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t n_keys = (size_t)key_off[n_sets];
    const agg_sum_plan p = musig_agg_plan_sum(key_off, n_sets, fold_fanin(e));
    stage_buf b[] = {{nullptr, results, 4 * n_sets}, {nullptr, out, pubkey_bytes(out_format) * n_sets}, {nullptr, parities_out, n_sets},
                     {keys, nullptr, pubkey_bytes(key_format) * n_keys, 64}};
    if (!stage_open(e, b, 0, combine_ws(p, combine_fused(key_format)))) return 0;
    stream_guard sg(e, e->stream);
    ws_carver w{e->ws, stage_bytes(b)};
    return stage_close(e, b, combine_run(e, e->stream, w, p, b[0].at<int32_t>(), b[1].at(), out_format, parities_out ? b[2].at() : nullptr, b[3].at(), key_format, n_sets));
}
