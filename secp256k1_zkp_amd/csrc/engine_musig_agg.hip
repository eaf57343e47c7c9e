#include "engine_lanes.h"
#include "musig_agg.h"

// ------------------------------------------------------------------------------------------------------------
// MuSig2, the rest of the coordinator's flow (musig_agg.h): key aggregation, the cache tweaks, nonce aggregation, signature aggregation
// ------------------------------------------------------------------------------------------------------------
// Key aggregation is a launch chain on the caller's stream, planned on the host from the set offsets: (a) one set per lane, (b) one key
// per lane over the flat key array, (c) the segmented sum, repeated until one partial per set is left, (d) one set per lane.  Nonce
// aggregation runs the same sum over its two columns (2 * n_sessions segments).  Offsets travel to the workspace as they are.

// (a)
__global__ void __launch_bounds__(256)
k_musig_agg_list(unsigned char* __restrict__ pks_hash, u32* __restrict__ second, const unsigned char* __restrict__ pks, int pk_format, const u64* __restrict__ set_off,
                 musig_agg_mids mid, size_t n_sets) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_sets) return;
    musig_agg_list_lane(pks_hash + 32 * k, second + k, mid.list, pks, pk_format, set_off[k], set_off[k + 1] - set_off[k]);
}

// (b) lanes [i0, i0 + m) of the flat key array (no lane leaves early: ecmult_lane builds its tables in lock step)
__global__ void __launch_bounds__(256, 2)
k_musig_agg_term(u32* __restrict__ partial, int32_t* __restrict__ key_ok, const unsigned char* __restrict__ pks, int pk_format, const u64* __restrict__ set_off, size_t n_sets,
                 const unsigned char* __restrict__ pks_hash, const u32* __restrict__ second, musig_agg_mids mid, const u32* __restrict__ gtab, u32* __restrict__ ptab,
                 size_t i0, size_t m) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < m;
    // Lane -> key: the first half of the launch takes the even keys, the second half the odd ones.  Any bijection is correct; this one
    // puts the second keys of a batch of 2-key sets (coefficient 1: no multiplication) into wavefronts of their own, which then skip
    // ecmult_lane's tables and loop altogether, instead of idling beside a first key in every wavefront.
    const size_t half = (m + 1) / 2;
    const size_t i = i0 + (live ? (lane < half ? 2 * lane : 2 * (lane - half) + 1) : 0);
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + lane * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const size_t k = (size_t)musig_agg_segment(set_off, n_sets, i);
    const int r = musig_agg_term_lane(partial + (size_t)MUSIG_AGG_GEJ_WORDS * i, mid.coef, pks, pk_format, i, set_off[k], second[k], pks_hash + 32 * k, live, gtab, lm);
    if (live) key_ok[i] = r;
}

// (c) outputs [j0, j0 + m): output j of segment k folds inputs in_off[k] + fanin * (j - out_off[k]) ...
__global__ void __launch_bounds__(256)
k_musig_agg_sum(u32* __restrict__ out, const u32* __restrict__ in, const u64* __restrict__ in_off, const u64* __restrict__ out_off, size_t nseg, unsigned fanin,
                size_t j0, size_t m) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= m) return;
    musig_agg_sum_item(out, in, in_off, out_off, nseg, fanin, j0 + lane);
}

// (d) (no lane leaves early: the to-affine inversion is shared by the 64 lanes of a wavefront)
__global__ void __launch_bounds__(256)
k_musig_agg_finish(int32_t* __restrict__ results, unsigned char* __restrict__ caches, unsigned char* __restrict__ agg_pks, const u32* __restrict__ sums,
                   const int32_t* __restrict__ key_ok, const u64* __restrict__ set_off, const unsigned char* __restrict__ pks_hash, const u32* __restrict__ second,
                   const unsigned char* __restrict__ pks, int pk_format, size_t n_sets) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < n_sets;
    const size_t k = live ? lane : 0;
    const u64 first = set_off[k], m = live ? set_off[k + 1] - first : 0;
    const int r = musig_agg_finish_lane(caches + (size_t)MUSIG_CACHE_BYTES * k, agg_pks ? agg_pks + 64 * k : nullptr, sums + (size_t)MUSIG_AGG_GEJ_WORDS * k, key_ok, first, m,
                                        pks_hash + 32 * k, second[k], pks, pk_format, live);
    if (live) results[k] = r;
}

// the cache tweaks (caches_out may be caches_in: no __restrict__ on the two)
__global__ void __launch_bounds__(256)
k_musig_agg_tweak(int32_t* __restrict__ results, unsigned char* caches_out, unsigned char* __restrict__ pks_out, const unsigned char* caches_in,
                  const unsigned char* __restrict__ tweaks, const unsigned char* __restrict__ xonly, const u32* __restrict__ gtab, size_t n) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < n;
    const size_t i = live ? lane : 0;
    const int r = musig_agg_tweak_lane(caches_out + (size_t)MUSIG_CACHE_BYTES * i, pks_out ? pks_out + 64 * i : nullptr, caches_in + (size_t)MUSIG_CACHE_BYTES * i, tweaks + 32 * i,
                                       xonly ? (unsigned)xonly[i] : 0u, live, gtab);
    if (live) results[i] = r;
}

// nonce aggregation: column 1 of pubnonce i at partial i, column 2 at partial n + i
__global__ void __launch_bounds__(256)
k_musig_agg_nonce_load(u32* __restrict__ partial, int32_t* __restrict__ nonce_ok, const unsigned char* __restrict__ nonces, int nonce_format, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    nonce_ok[i] = musig_agg_nonce_load_lane(partial + (size_t)MUSIG_AGG_GEJ_WORDS * i, partial + (size_t)MUSIG_AGG_GEJ_WORDS * (n + i), nonces + musig_nonce_bytes(nonce_format) * i,
                                            nonce_format, 1);
}
__global__ void __launch_bounds__(256)
k_musig_agg_nonce_finish(int32_t* __restrict__ results, unsigned char* __restrict__ out, int out_format, const u32* __restrict__ sums, const int32_t* __restrict__ nonce_ok,
                         const u64* __restrict__ nonce_off, size_t n_sessions) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = lane < n_sessions;
    const size_t k = live ? lane : 0;
    const u64 first = nonce_off[k], m = live ? nonce_off[k + 1] - first : 0;
    const int r = musig_agg_nonce_finish_lane(out + musig_nonce_bytes(out_format) * k, out_format, sums + (size_t)MUSIG_AGG_GEJ_WORDS * k,
                                              sums + (size_t)MUSIG_AGG_GEJ_WORDS * (n_sessions + k), nonce_ok, first, m, live);
    if (live) results[k] = r;
}

__global__ void __launch_bounds__(256)
k_musig_agg_sig(int32_t* __restrict__ results, unsigned char* __restrict__ sigs_out, const unsigned char* __restrict__ sessions, const unsigned char* __restrict__ sigs,
                int sig_format, const u64* __restrict__ sig_off, size_t n_sessions) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_sessions) return;
    results[k] = musig_agg_sig_lane(sigs_out + 64 * k, sessions + (size_t)MUSIG_SESSION_BYTES * k, sigs, sig_format, sig_off[k], sig_off[k + 1] - sig_off[k], 1);
}

// ---- host plans ------------------------------------------------------------------------------------------------------------------------
static int agg_offsets_ok(const char* who, const uint64_t* off, size_t n) {
    if (off[0] != 0) return s2k_fail_arg(who, "offsets must start at 0");
    for (size_t k = 0; k < n; k++) if (off[k + 1] < off[k]) return s2k_fail_arg(who, "offsets must not decrease");
    return 1;
}
typedef musig_agg_sum_plan agg_sum_plan;      // (musig_agg.h)
static size_t agg_sum_ws(const agg_sum_plan& p) { return ws_need({8 * p.offs.size(), (size_t)4 * MUSIG_AGG_GEJ_WORDS * p.cap, (size_t)4 * MUSIG_AGG_GEJ_WORDS * p.cap}); }
static agg_sum_bufs agg_sum_carve(ws_carver& w, const agg_sum_plan& p) {
    agg_sum_bufs s; s.d_off = w.take<u64>(p.offs.size()); s.a = w.take<u32>((size_t)MUSIG_AGG_GEJ_WORDS * p.cap); s.b = w.take<u32>((size_t)MUSIG_AGG_GEJ_WORDS * p.cap);
    return s;
}
// runs the passes from `first_pass` on (engine_internal.h: also offered to engine_pubkey.hip, whose own kernel is pass 0); pass q reads
// s.a when q is even and s.b when it is odd.  *result is where the nseg sums are.
int agg_sum_launch(s2k_engine* e, hipStream_t st, const agg_sum_plan& p, const agg_sum_bufs& s, unsigned fanin, const u32** result, size_t first_pass) {
    u32* in = s.a; u32* out = s.b;
    if (first_pass & 1) std::swap(in, out);
    for (size_t q = first_pass; q < p.passes; q++) {
        const u64* in_off = s.d_off + q * (p.nseg + 1); const u64* out_off = in_off + p.nseg + 1;
        const size_t total = (size_t)p.offs[(q + 1) * (p.nseg + 1) + p.nseg];
        for (size_t j0 = 0; j0 < total; j0 += e->max_lanes) {
            const size_t m = std::min(total - j0, e->max_lanes);
            hipLaunchKernelGGL(k_musig_agg_sum, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out, (const u32*)in, in_off, out_off, p.nseg, fanin, j0, m);
        }
        std::swap(in, out);
    }
    HIPCHK(hipGetLastError());
    *result = in;
    return 1;
}
// The offset arrays reach the workspace by hipMemcpyAsync on the caller's stream (ordered behind earlier calls that still read the
// workspace) from PAGEABLE host memory -- a std::vector of this file, never the caller's array, which may be pinned: the runtime
// stages a pageable source before hipMemcpyAsync returns, which is what lets the vector die and the caller reuse its offsets when
// the entry point returns ("read before the call returns"; s2k_ecmult_multi_many_dev relies on the same).
static unsigned agg_fanin(const s2k_engine* e) { return e->musig_sum_fanin ? (unsigned)e->musig_sum_fanin : (unsigned)MUSIG_AGG_FANIN_DEFAULT; }

// ---- key aggregation -------------------------------------------------------------------------------------------------------------------
static size_t keyagg_ws(const agg_sum_plan& p, size_t n_keys, size_t n_sets) { return agg_sum_ws(p) + ws_need({4 * n_keys, 32 * n_sets, 4 * n_sets}); }
// every array on the device; the carver continues behind whatever the caller staged
static int keyagg_run(s2k_engine* e, hipStream_t st, ws_carver& w, const agg_sum_plan& p, int32_t* results, unsigned char* caches, unsigned char* agg_pks,
                      const unsigned char* pks, int pk_format, size_t n_sets) {
    const size_t n_keys = (size_t)p.offs[n_sets];
    const agg_sum_bufs s = agg_sum_carve(w, p);
    int32_t* key_ok = w.take<int32_t>(n_keys); unsigned char* pks_hash = w.take<unsigned char>(32 * n_sets); u32* second = w.take<u32>(n_sets);
    const size_t lanes = ((std::min(std::max(n_keys, (size_t)1), e->max_lanes) + 255) / 256) * 256;
    if (!engine_ptab(e, lanes)) return 0;
    ENGINE_GTAB(e, st);
    musig_agg_mids mid; musig_agg_midstates(mid);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n_sets, st));
    HIPCHK(hipMemsetAsync(caches, 0, (size_t)MUSIG_CACHE_BYTES * n_sets, st));
    if (agg_pks) HIPCHK(hipMemsetAsync(agg_pks, 0, 64 * n_sets, st));
    HIPCHK(hipMemcpyAsync(s.d_off, p.offs.data(), 8 * p.offs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st));
    hipLaunchKernelGGL(k_musig_agg_list, dim3((unsigned)((n_sets + 255) / 256)), dim3(256), 0, st, pks_hash, second, pks, pk_format, (const u64*)s.d_off, mid, n_sets);
    HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n_keys; i0 += e->max_lanes) {
        const size_t m = std::min(n_keys - i0, e->max_lanes);
        hipLaunchKernelGGL(k_musig_agg_term, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, s.a, key_ok, pks, pk_format, (const u64*)s.d_off, n_sets,
                           (const unsigned char*)pks_hash, (const u32*)second, mid, (const u32*)e->gtab, e->ptab, i0, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st));
    const u32* sums = nullptr;
    if (!agg_sum_launch(e, st, p, s, agg_fanin(e), &sums)) return 0;
    hipLaunchKernelGGL(k_musig_agg_finish, dim3((unsigned)((n_sets + 255) / 256)), dim3(256), 0, st, results, caches, agg_pks, sums, (const int32_t*)key_ok,
                       (const u64*)s.d_off, (const unsigned char*)pks_hash, (const u32*)second, pks, pk_format, n_sets);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
// what the entry points check behind their NULL checks of results, outputs and offsets (the host forms zero their outputs in between)
static int keyagg_args(const char* who, const unsigned char* pks, int pk_format, const uint64_t* set_off, size_t n_sets) {
    if (set_off[n_sets] && !pks) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (pk_format < 0 || pk_format > 2) return s2k_fail_arg(who, "pk_format must be 0 (compressed), 1 (object) or 2 (uncompressed / hybrid)");
    return agg_offsets_ok(who, set_off, n_sets);
}

extern "C" int secp256k1_musig_pubkey_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* caches_out197, unsigned char* agg_pks_out64,
                                                    const unsigned char* pubkeys, int pk_format, const uint64_t* set_off, size_t n_sets) {
    const char* who = "secp256k1_musig_pubkey_agg_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sets == 0) return 1;
    if (!results || !caches_out197 || !set_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!keyagg_args(who, pubkeys, pk_format, set_off, n_sets)) return 0;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const agg_sum_plan p = musig_agg_plan_sum(set_off, n_sets, agg_fanin(e));
    if (!engine_workspace(e, keyagg_ws(p, (size_t)set_off[n_sets], n_sets))) return 0;
    ws_carver w{e->ws, 0};
    return keyagg_run(e, st, w, p, results, caches_out197, agg_pks_out64, pubkeys, pk_format, n_sets);
}
extern "C" int secp256k1_musig_pubkey_agg_batch(s2k_engine* e, int32_t* results, unsigned char* caches_out197, unsigned char* agg_pks_out64, const unsigned char* pubkeys,
                                                int pk_format, const uint64_t* set_off, size_t n_sets) {
    const char* who = "secp256k1_musig_pubkey_agg_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sets == 0) return 1;
    if (!results || !caches_out197 || !set_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n_sets);
    memset(caches_out197, 0, (size_t)MUSIG_CACHE_BYTES * n_sets);
    if (agg_pks_out64) memset(agg_pks_out64, 0, 64 * n_sets);
    if (!keyagg_args(who, pubkeys, pk_format, set_off, n_sets)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t n_keys = (size_t)set_off[n_sets], pkb = ecdsa_pk_bytes(pk_format), cb = (size_t)MUSIG_CACHE_BYTES * n_sets;
    const agg_sum_plan p = musig_agg_plan_sum(set_off, n_sets, agg_fanin(e));
    stage_buf b[] = {{nullptr, results, 4 * n_sets}, {nullptr, caches_out197, cb}, {nullptr, agg_pks_out64, 64 * n_sets}, {pubkeys, nullptr, pkb * n_keys}};
    if (!stage_open(e, b, 0, keyagg_ws(p, n_keys, n_sets))) return 0;
    stream_guard sg(e, e->stream);
    ws_carver w{e->ws, stage_bytes(b)};
    return stage_close(e, b, keyagg_run(e, e->stream, w, p, b[0].at<int32_t>(), b[1].at(), agg_pks_out64 ? b[2].at() : nullptr, b[3].at(), pk_format, n_sets));
}

// ---- the cache tweaks --------------------------------------------------------------------------------------------------------------------
extern "C" int secp256k1_musig_pubkey_tweak_add_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* caches_out197, unsigned char* pubkeys_out64,
                                                          const unsigned char* caches_in197, const unsigned char* tweaks32, const unsigned char* xonly, size_t n) {
    const char* who = "secp256k1_musig_pubkey_tweak_add_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !caches_out197 || !caches_in197 || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    ENGINE_GTAB(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));
    if (caches_out197 != caches_in197) HIPCHK(hipMemsetAsync(caches_out197, 0, (size_t)MUSIG_CACHE_BYTES * n, st));      // (in place: the kernel writes the zeros)
    if (pubkeys_out64) HIPCHK(hipMemsetAsync(pubkeys_out64, 0, 64 * n, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_musig_agg_tweak, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, caches_out197 + (size_t)MUSIG_CACHE_BYTES * i0,
                           pubkeys_out64 ? pubkeys_out64 + 64 * i0 : nullptr, caches_in197 + (size_t)MUSIG_CACHE_BYTES * i0, tweaks32 + 32 * i0, xonly ? xonly + i0 : nullptr,
                           (const u32*)e->gtab, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_musig_pubkey_tweak_add_batch(s2k_engine* e, int32_t* results, unsigned char* caches_out197, unsigned char* pubkeys_out64,
                                                      const unsigned char* caches_in197, const unsigned char* tweaks32, const unsigned char* xonly, size_t n) {
    const char* who = "secp256k1_musig_pubkey_tweak_add_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !caches_out197 || !caches_in197 || !tweaks32) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    const size_t cb = (size_t)MUSIG_CACHE_BYTES * n;
    // a call that does not complete leaves zeroed outputs, as the other host forms -- except the caches of an in-place call, which
    // are its input as well: they stay as they were unless the device call itself was reached and failed
    memset(results, 0, sizeof(int32_t) * n);
    if (caches_out197 != caches_in197) memset(caches_out197, 0, cb);
    if (pubkeys_out64) memset(pubkeys_out64, 0, 64 * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    // (the caches are tweaked in place on the device: one buffer, uploaded and downloaded)
    stage_buf b[] = {{nullptr, results, 4 * n}, {caches_in197, caches_out197, cb}, {nullptr, pubkeys_out64, 64 * n}, {tweaks32, nullptr, 32 * n}, {xonly, nullptr, n}};
    if (!stage_open(e, b)) return 0;
    if (!secp256k1_musig_pubkey_tweak_add_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), pubkeys_out64 ? b[2].at() : nullptr, b[1].at(), b[3].at(), b[4].opt(), n)) {
        (void)stage_close(e, b, 0); memset(caches_out197, 0, cb); if (pubkeys_out64) memset(pubkeys_out64, 0, 64 * n); return 0;
    }
    return stage_close(e, b, 1);
}

// ---- nonce aggregation -------------------------------------------------------------------------------------------------------------------
static size_t nonce_agg_ws(const agg_sum_plan& p, size_t n_nonces) { return agg_sum_ws(p) + ws_need({4 * n_nonces}); }
static int nonce_agg_run(s2k_engine* e, hipStream_t st, ws_carver& w, const agg_sum_plan& p, int32_t* results, unsigned char* out, int out_format,
                         const unsigned char* nonces, int nonce_format, size_t n_sessions) {
    const size_t n = (size_t)p.offs[n_sessions];
    const agg_sum_bufs s = agg_sum_carve(w, p);
    int32_t* nonce_ok = w.take<int32_t>(n);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n_sessions, st));
    HIPCHK(hipMemsetAsync(out, 0, musig_nonce_bytes(out_format) * n_sessions, st));
    HIPCHK(hipMemcpyAsync(s.d_off, p.offs.data(), 8 * p.offs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    if (n) hipLaunchKernelGGL(k_musig_agg_nonce_load, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.a, nonce_ok, nonces, nonce_format, n);
    const u32* sums = nullptr;
    if (!agg_sum_launch(e, st, p, s, agg_fanin(e), &sums)) return 0;
    HIPCHK(hipEventRecord(e->ev[3], st));
    hipLaunchKernelGGL(k_musig_agg_nonce_finish, dim3((unsigned)((n_sessions + 255) / 256)), dim3(256), 0, st, results, out, out_format, sums, (const int32_t*)nonce_ok,
                       (const u64*)s.d_off, n_sessions);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
static int nonce_agg_args(const char* who, int out_format, const unsigned char* nonces, int nonce_format, const uint64_t* nonce_off, size_t n_sessions) {
    if (nonce_off[n_sessions] && !nonces) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (out_format < 0 || out_format > 1) return s2k_fail_arg(who, "out_format must be 0 (66 bytes serialised) or 1 (132-byte object)");
    if (nonce_format < 0 || nonce_format > 1) return s2k_fail_arg(who, "nonce_format must be 0 (66 bytes serialised) or 1 (132-byte object)");
    return agg_offsets_ok(who, nonce_off, n_sessions);
}
extern "C" int secp256k1_musig_nonce_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggnonces_out, int out_format, const unsigned char* pubnonces,
                                                   int nonce_format, const uint64_t* nonce_off, size_t n_sessions) {
    const char* who = "secp256k1_musig_nonce_agg_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sessions == 0) return 1;
    if (!results || !aggnonces_out || !nonce_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!nonce_agg_args(who, out_format, pubnonces, nonce_format, nonce_off, n_sessions)) return 0;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const agg_sum_plan p = musig_agg_plan_nonces(nonce_off, n_sessions, agg_fanin(e));
    if (!engine_workspace(e, nonce_agg_ws(p, (size_t)nonce_off[n_sessions]))) return 0;
    ws_carver w{e->ws, 0};
    return nonce_agg_run(e, st, w, p, results, aggnonces_out, out_format, pubnonces, nonce_format, n_sessions);
}
extern "C" int secp256k1_musig_nonce_agg_batch(s2k_engine* e, int32_t* results, unsigned char* aggnonces_out, int out_format, const unsigned char* pubnonces, int nonce_format,
                                               const uint64_t* nonce_off, size_t n_sessions) {
    const char* who = "secp256k1_musig_nonce_agg_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sessions == 0) return 1;
    if (!results || !aggnonces_out || !nonce_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n_sessions);
    if (out_format == 0 || out_format == 1) memset(aggnonces_out, 0, musig_nonce_bytes(out_format) * n_sessions);
    if (!nonce_agg_args(who, out_format, pubnonces, nonce_format, nonce_off, n_sessions)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)nonce_off[n_sessions], nb = musig_nonce_bytes(nonce_format), ob = musig_nonce_bytes(out_format) * n_sessions;
    const agg_sum_plan p = musig_agg_plan_nonces(nonce_off, n_sessions, agg_fanin(e));
    stage_buf b[] = {{nullptr, results, 4 * n_sessions}, {nullptr, aggnonces_out, ob}, {pubnonces, nullptr, nb * n}};
    if (!stage_open(e, b, 0, nonce_agg_ws(p, n))) return 0;
    stream_guard sg(e, e->stream);
    ws_carver w{e->ws, stage_bytes(b)};
    return stage_close(e, b, nonce_agg_run(e, e->stream, w, p, b[0].at<int32_t>(), b[1].at(), out_format, b[2].at(), nonce_format, n_sessions));
}

// ---- signature aggregation -----------------------------------------------------------------------------------------------------------------
static int sig_agg_run(s2k_engine* e, hipStream_t st, ws_carver& w, int32_t* results, unsigned char* sigs_out, const unsigned char* sessions, const unsigned char* sigs,
                       int sig_format, const uint64_t* sig_off, size_t n_sessions) {
    u64* d_off = w.take<u64>(n_sessions + 1);
    const std::vector<uint64_t> off(sig_off, sig_off + n_sessions + 1);      // (pageable whatever the caller's array is: see agg_fanin's note)
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n_sessions, st));
    HIPCHK(hipMemsetAsync(sigs_out, 0, 64 * n_sessions, st));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), 8 * (n_sessions + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    hipLaunchKernelGGL(k_musig_agg_sig, dim3((unsigned)((n_sessions + 255) / 256)), dim3(256), 0, st, results, sigs_out, sessions, sigs, sig_format, (const u64*)d_off, n_sessions);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
static int sig_agg_args(const char* who, const unsigned char* sigs, int sig_format, const uint64_t* sig_off, size_t n_sessions) {
    if (sig_off[n_sessions] && !sigs) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (sig_format < 0 || sig_format > 1) return s2k_fail_arg(who, "sig_format must be 0 (32 bytes serialised) or 1 (36-byte object)");
    return agg_offsets_ok(who, sig_off, n_sessions);
}
extern "C" int secp256k1_musig_partial_sig_agg_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* sigs64_out, const unsigned char* sessions133,
                                                         const unsigned char* partial_sigs, int sig_format, const uint64_t* sig_off, size_t n_sessions) {
    const char* who = "secp256k1_musig_partial_sig_agg_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sessions == 0) return 1;
    if (!results || !sigs64_out || !sessions133 || !sig_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!sig_agg_args(who, partial_sigs, sig_format, sig_off, n_sessions)) return 0;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!engine_workspace(e, ws_need({8 * (n_sessions + 1)}))) return 0;
    ws_carver w{e->ws, 0};
    return sig_agg_run(e, st, w, results, sigs64_out, sessions133, partial_sigs, sig_format, sig_off, n_sessions);
}
extern "C" int secp256k1_musig_partial_sig_agg_batch(s2k_engine* e, int32_t* results, unsigned char* sigs64_out, const unsigned char* sessions133,
                                                     const unsigned char* partial_sigs, int sig_format, const uint64_t* sig_off, size_t n_sessions) {
    const char* who = "secp256k1_musig_partial_sig_agg_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n_sessions == 0) return 1;
    if (!results || !sigs64_out || !sessions133 || !sig_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n_sessions);
    memset(sigs64_out, 0, 64 * n_sessions);
    if (!sig_agg_args(who, partial_sigs, sig_format, sig_off, n_sessions)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)sig_off[n_sessions], sgb = musig_sig_bytes(sig_format), sb = (size_t)MUSIG_SESSION_BYTES * n_sessions;
    stage_buf b[] = {{nullptr, results, 4 * n_sessions}, {nullptr, sigs64_out, 64 * n_sessions}, {sessions133, nullptr, sb}, {partial_sigs, nullptr, sgb * n}};
    if (!stage_open(e, b, 0, 8 * (n_sessions + 1))) return 0;      // (the runner's offsets)
    stream_guard sg(e, e->stream);
    ws_carver w{e->ws, stage_bytes(b)};
    return stage_close(e, b, sig_agg_run(e, e->stream, w, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].at(), sig_format, sig_off, n_sessions));
}
