#include "engine_lanes.h"
#include "halfagg_batch.h"

// ------------------------------------------------------------------------------------------------------------
// half-aggregated Schnorr signatures, many aggregates per call (halfagg_batch.h): batch verification as K sums in one launch chain
// (engine_msm_many.hip) behind one hash chain per LANE, and batch (incremental) aggregation
// ------------------------------------------------------------------------------------------------------------
// The chain kernel is the serial floor of both: lane L walks aggregate perm[L] (aggregates sorted by length on the host, so that a
// wavefront's lanes finish together).  One wavefront per workgroup: a batch of a few thousand aggregates is a few dozen wavefronts, and
// they should land on different CUs.  r_off NULL: aggregate k's r_j are at byte 32 (item_off[k] + k) of r_base (the aggregator's output).
__global__ void __launch_bounds__(64)
k_hab_chain(u32* __restrict__ states, const unsigned char* __restrict__ r_base, const u64* __restrict__ r_off, const unsigned char* __restrict__ pks, int pk_format,
            const unsigned char* __restrict__ msgs32, const u64* __restrict__ item_off, const u32* __restrict__ perm, size_t m) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= m) return;
    const size_t k = perm[lane];
    const u64 first = item_off[k], n = item_off[k + 1] - first;
    hab_chain_lane(states + 8 * hab_state_slot(first), r_base + (r_off ? r_off[k] : 32 * (first + k)), pks + (pk_format ? 64 : 32) * first, pk_format, msgs32 + 32 * first,
                   (size_t)n);
}
__global__ void __launch_bounds__(256)
k_hab_points(hab_verify_view v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hab_points_item(v, i);
}
__global__ void __launch_bounds__(256)
k_hab_scalars(hab_verify_view v, schnorr_midstate bip340, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hab_scalars_item(v, bip340, i);
}
__global__ void __launch_bounds__(256)
k_hab_gscalar(hab_verify_view v) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < v.n_aggs) hab_gscalar_agg(v, k);
}
__global__ void __launch_bounds__(256)
k_hab_final(int32_t* __restrict__ results, hab_verify_view v, const int32_t* __restrict__ r_inf, u64 max_terms) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.n_aggs) return;
    const int r = hab_verdict(v.item_off, v.agg_off, k, max_terms, v.fail[k], r_inf[k]);
    if (r >= 0) results[k] = r;                              // (an over-limit aggregate's verdict comes from the single-aggregate path)
}
__global__ void __launch_bounds__(256)
k_hab_gather(hab_agg_view v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hab_gather_item(v, i);
}
__global__ void __launch_bounds__(256)
k_hab_term(hab_agg_view v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hab_term_item(v, i);
}
__global__ void __launch_bounds__(256)
k_hab_sum(int32_t* __restrict__ results, hab_agg_view v) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < v.n_aggs) results[k] = hab_sum_agg(v, k);
}
static inline dim3 hab_grid(size_t n, unsigned block) { return dim3((unsigned)((n + block - 1) / block)); }

// ---- verification ------------------------------------------------------------------------------------------------------------------------
// The offsets travel as ONE pageable vector of this file (item_off | agg_off | moff): see the note above agg_fanin in engine_musig_agg.hip.
struct hab_verify_sizes { size_t K, N, NT, NP; };
static size_t hab_verify_carve_bytes(const hab_verify_sizes& z) {
    return ws_need({8 * 3 * (z.K + 1), 4 * z.NP + 64, 128 * z.NT + 64, 64 * z.NT + 64, 32 * z.K + 64, 32 * z.N + 64, 32 * (hab_state_slot(z.N) + 1), 4 * z.K + 64, 64 * z.K + 64,
                    4 * z.K + 64}) + 256;      // (+ 256: what follows starts at the next 256-byte boundary)
}
// workspace of one call, behind the staged inputs where the host form runs it
static size_t hab_verify_ws(const s2k_engine* e, const hab_verify_sizes& z, const hab_verify_plan& p, const uint64_t* item_off) {
    size_t tail = mm_ws_bytes(e, p.moff.data(), z.K, 1u);
    for (u32 k : p.large) tail = std::max(tail, ha_ws_bytes(e, (size_t)(item_off[k + 1] - item_off[k])));
    return hab_verify_carve_bytes(z) + tail;
}
static hab_verify_sizes hab_sizes(const uint64_t* item_off, size_t K, const hab_verify_plan& p) {
    return hab_verify_sizes{K, (size_t)item_off[K], (size_t)(p.moff[K] >> 1), p.perm.size()};
}
// every byte array on the device; results zeroed on the stream first
static int hab_verify_run(s2k_engine* e, hipStream_t st, size_t front, int32_t* results, const unsigned char* pks, int pk_format, const unsigned char* msgs32,
                          const unsigned char* aggsigs, const uint64_t* item_off, const uint64_t* agg_off, size_t K, const hab_verify_plan& p) {
    const hab_verify_sizes z = hab_sizes(item_off, K, p);
    ws_carver c{e->ws, front};
    u64* d_off = c.take<u64>(3 * (K + 1)); u32* d_perm = c.take<u32>(z.NP + 16);
    unsigned char* d_pts = c.take<unsigned char>(128 * z.NT + 64); unsigned char* d_sc = c.take<unsigned char>(64 * z.NT + 64);
    unsigned char* d_g = c.take<unsigned char>(32 * K + 64); unsigned char* d_pkx = c.take<unsigned char>(32 * z.N + 64);
    u32* d_states = c.take<u32>(8 * (hab_state_slot(z.N) + 1)); u32* d_fail = c.take<u32>(K + 16);
    unsigned char* d_rxy = c.take<unsigned char>(64 * K + 64); int32_t* d_rinf = c.take<int32_t>(K + 16);
    const size_t tail = (c.off + 255) & ~size_t(255);
    std::vector<uint64_t> offs(3 * (K + 1));
    for (size_t k = 0; k <= K; k++) { offs[k] = item_off[k]; offs[K + 1 + k] = agg_off[k]; offs[2 * (K + 1) + k] = p.moff[k]; }
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * K, st));
    HIPCHK(hipMemsetAsync(d_fail, 0, sizeof(u32) * K, st));
    HIPCHK(hipMemcpyAsync(d_off, offs.data(), 8 * offs.size(), hipMemcpyHostToDevice, st));
    if (z.NP) HIPCHK(hipMemcpyAsync(d_perm, p.perm.data(), 4 * z.NP, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st));
    const hab_verify_view v{d_off, d_off + (K + 1), d_off + 2 * (K + 1), K, pks, pk_format, msgs32, aggsigs, d_pts, d_sc, d_g, d_pkx, d_states, d_fail};
    if (z.NP) hipLaunchKernelGGL(k_hab_chain, hab_grid(z.NP, 64), dim3(64), 0, st, d_states, aggsigs, v.agg_off, pks, pk_format, msgs32, v.item_off, (const u32*)d_perm, z.NP);
    if (z.N) hipLaunchKernelGGL(k_hab_points, hab_grid(z.N, 256), dim3(256), 0, st, v, z.N);
    if (z.N) hipLaunchKernelGGL(k_hab_scalars, hab_grid(z.N, 256), dim3(256), 0, st, v, e->bip340, z.N);
    hipLaunchKernelGGL(k_hab_gscalar, hab_grid(K, 256), dim3(256), 0, st, v);
    HIPCHK(hipGetLastError());
    // the K sums: points R_0, P_0, R_1, P_1, ... and scalars z_0, z_0 e_0, ... of every aggregate of the batch, its generator term -s_k
    if (!mm_impl(e, st, tail, d_rxy, d_rinf, d_g, d_sc, d_pts, nullptr, p.moff.data(), K)) return 0;
    hipLaunchKernelGGL(k_hab_final, hab_grid(K, 256), dim3(256), 0, st, results, v, (const int32_t*)d_rinf, (u64)MM_MAX_TERMS);
    HIPCHK(hipGetLastError());
    // over the limit: one (2 n + 1)-term MSM each, behind the batch (the same workspace region, stream-ordered)
    for (u32 k : p.large) {
        ws_carver cl{e->ws, tail};
        const size_t first = (size_t)item_off[k];
        if (!ha_launch(e, st, cl, results + k, pks + (pk_format ? 64 : 32) * first, pk_format, msgs32 + 32 * first, (size_t)(item_off[k + 1] - item_off[k]), aggsigs + agg_off[k])) return 0;
    }
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
static int hab_verify_args(const char* who, const unsigned char* pks, int pk_format, const unsigned char* msgs32, const uint64_t* item_off, const uint64_t* agg_off, size_t K) {
    if (pk_format < 0 || pk_format > 1) return s2k_fail_arg(who, "pk_format must be 0 (32-byte x-only keys) or 1 (64-byte objects)");
    if (!mm_check_offsets(who, item_off, K) || !mm_check_offsets(who, agg_off, K)) return 0;
    if (item_off[K] && (!pks || !msgs32)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (item_off[K] >= (uint64_t(1) << 40) || agg_off[K] >= (uint64_t(1) << 46) || K >= (size_t(1) << 31)) return s2k_fail_arg(who, "batch too large");
    return 1;
}
extern "C" int secp256k1_schnorrsig_aggverify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                        const uint64_t* item_off, const unsigned char* aggsigs, const uint64_t* aggsig_off, size_t n_aggs) {
    const char* who = "secp256k1_schnorrsig_aggverify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n_aggs == 0) return 1;
    if (!results || !aggsigs || !item_off || !aggsig_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!hab_verify_args(who, pubkeys, pk_format, msgs32, item_off, aggsig_off, n_aggs)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const hab_verify_plan p = hab_plan_verify(item_off, aggsig_off, n_aggs, MM_MAX_TERMS);
    if (!engine_workspace(e, hab_verify_ws(e, hab_sizes(item_off, n_aggs, p), p, item_off))) return 0;
    return hab_verify_run(e, st, 0, results, pubkeys, pk_format, msgs32, aggsigs, item_off, aggsig_off, n_aggs, p);
}
extern "C" int secp256k1_schnorrsig_aggverify_batch(s2k_engine* e, int32_t* results, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                    const uint64_t* item_off, const unsigned char* aggsigs, const uint64_t* aggsig_off, size_t n_aggs) {
    const char* who = "secp256k1_schnorrsig_aggverify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n_aggs == 0) return 1;
    if (!results || !aggsigs || !item_off || !aggsig_off) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n_aggs);
    if (!hab_verify_args(who, pubkeys, pk_format, msgs32, item_off, aggsig_off, n_aggs)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t K = n_aggs, N = (size_t)item_off[K], A = (size_t)aggsig_off[K], pkb = pk_format ? 64 : 32;
    const hab_verify_plan p = hab_plan_verify(item_off, aggsig_off, K, MM_MAX_TERMS);
    stage_buf b[] = {{pubkeys, nullptr, pkb * N, 64}, {msgs32, nullptr, 32 * N, 64}, {aggsigs, nullptr, A, 64}, {nullptr, results, 4 * K, 64}};
    if (!stage_open(e, b, 0, hab_verify_ws(e, hab_sizes(item_off, K, p), p, item_off))) return 0;
    stream_guard sg(e, st);
    return stage_close(e, b, hab_verify_run(e, st, stage_bytes(b), b[3].at<int32_t>(), b[0].at(), pk_format, b[1].at(), b[2].at(), item_off, aggsig_off, K, p));
}

// ---- aggregation -------------------------------------------------------------------------------------------------------------------------
// n_before NULL: the plain aggregation (every count 0, no aggsigs_in).  offs: item_off | in_off | new_off.
struct hab_agg_plan { std::vector<uint64_t> offs; std::vector<u32> perm; size_t K, N, in_bytes, n_new; };
static int hab_agg_make_plan(const char* who, hab_agg_plan& p, const uint64_t* item_off, const uint64_t* n_before, size_t K) {
    p.K = K; p.N = (size_t)item_off[K];
    p.offs.assign(3 * (K + 1), 0);
    std::vector<u32> all(K);
    for (size_t k = 0; k < K; k++) {
        const uint64_t n = item_off[k + 1] - item_off[k], nb = n_before ? n_before[k] : 0;
        if (nb > n) return s2k_fail_arg(who, "n_before[k] exceeds the aggregate's item count");
        p.offs[k] = item_off[k];
        p.offs[K + 1 + k + 1] = p.offs[K + 1 + k] + 32 * (nb + 1);
        p.offs[2 * (K + 1) + k + 1] = p.offs[2 * (K + 1) + k] + (n - nb);
        all[k] = (u32)k;
    }
    p.offs[K] = item_off[K];
    p.in_bytes = n_before ? (size_t)p.offs[2 * K + 1] : 0; p.n_new = (size_t)p.offs[3 * K + 2];
    p.perm = hab_chain_order(item_off, all);
    return 1;
}
static size_t hab_agg_ws(const hab_agg_plan& p) {
    return ws_need({8 * 3 * (p.K + 1), 4 * p.perm.size() + 64, 32 * p.N + 64, 32 * (hab_state_slot(p.N) + 1), 4 * p.K + 64});
}
static int hab_agg_run(s2k_engine* e, hipStream_t st, size_t front, int32_t* results, unsigned char* out, const unsigned char* aggsigs_in, int have_in, const unsigned char* pks,
                       int pk_format, const unsigned char* msgs32, const unsigned char* new_sigs64, const hab_agg_plan& p) {
    const size_t K = p.K, N = p.N, NP = p.perm.size();
    ws_carver c{e->ws, front};
    u64* d_off = c.take<u64>(3 * (K + 1)); u32* d_perm = c.take<u32>(NP + 16); unsigned char* d_t = c.take<unsigned char>(32 * N + 64);
    u32* d_states = c.take<u32>(8 * (hab_state_slot(N) + 1)); u32* d_fail = c.take<u32>(K + 16);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * K, st));
    HIPCHK(hipMemsetAsync(out, 0, 32 * (N + K), st));
    HIPCHK(hipMemsetAsync(d_fail, 0, sizeof(u32) * K, st));
    HIPCHK(hipMemcpyAsync(d_off, p.offs.data(), 8 * p.offs.size(), hipMemcpyHostToDevice, st));
    if (NP) HIPCHK(hipMemcpyAsync(d_perm, p.perm.data(), 4 * NP, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev[0], st));
    const hab_agg_view v{d_off, have_in ? d_off + (K + 1) : nullptr, d_off + 2 * (K + 1), K, pks, pk_format, msgs32, aggsigs_in, new_sigs64, out, d_t, d_states, d_fail};
    if (N) hipLaunchKernelGGL(k_hab_gather, hab_grid(N, 256), dim3(256), 0, st, v, N);
    HIPCHK(hipEventRecord(e->ev[2], st));
    if (NP) hipLaunchKernelGGL(k_hab_chain, hab_grid(NP, 64), dim3(64), 0, st, d_states, (const unsigned char*)out, (const u64*)nullptr, pks, pk_format, msgs32, v.item_off, (const u32*)d_perm, NP);
    HIPCHK(hipEventRecord(e->ev[3], st));
    if (N) hipLaunchKernelGGL(k_hab_term, hab_grid(N, 256), dim3(256), 0, st, v, N);
    hipLaunchKernelGGL(k_hab_sum, hab_grid(K, 256), dim3(256), 0, st, results, v);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
static int hab_agg_args(const char* who, const unsigned char* pks, int pk_format, const unsigned char* msgs32, const uint64_t* item_off, size_t K) {
    if (pk_format < 0 || pk_format > 1) return s2k_fail_arg(who, "pk_format must be 0 (32-byte x-only keys) or 1 (64-byte objects)");
    if (!mm_check_offsets(who, item_off, K)) return 0;
    if (item_off[K] && (!pks || !msgs32)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (item_off[K] >= (uint64_t(1) << 40) || K >= (size_t(1) << 31)) return s2k_fail_arg(who, "batch too large");
    return 1;
}
// both aggregation calls, device form (inc = 0: n_before and aggsigs_in are not looked at)
static int hab_agg_dev(const char* who, int inc, s2k_engine* e, void* stream, int32_t* results, unsigned char* out, const unsigned char* aggsigs_in, const uint64_t* n_before,
                       const unsigned char* pks, int pk_format, const unsigned char* msgs32, const unsigned char* new_sigs64, const uint64_t* item_off, size_t K) {
    if (!e) return s2k_fail(who, "null engine");
    if (K == 0) return 1;
    if (!results || !out || !item_off || (inc && (!aggsigs_in || !n_before))) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!hab_agg_args(who, pks, pk_format, msgs32, item_off, K)) return 0;
    hab_agg_plan p;
    if (!hab_agg_make_plan(who, p, item_off, inc ? n_before : nullptr, K)) return 0;
    if (p.n_new && !new_sigs64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!engine_workspace(e, hab_agg_ws(p))) return 0;
    return hab_agg_run(e, st, 0, results, out, aggsigs_in, inc, pks, pk_format, msgs32, new_sigs64, p);
}
static int hab_agg_host(const char* who, int inc, s2k_engine* e, int32_t* results, unsigned char* out, const unsigned char* aggsigs_in, const uint64_t* n_before,
                        const unsigned char* pks, int pk_format, const unsigned char* msgs32, const unsigned char* new_sigs64, const uint64_t* item_off, size_t K) {
    if (!e) return s2k_fail(who, "null engine");
    if (K == 0) return 1;
    if (!results || !out || !item_off || (inc && (!aggsigs_in || !n_before))) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * K);
    if (!hab_agg_args(who, pks, pk_format, msgs32, item_off, K)) return 0;
    memset(out, 0, 32 * ((size_t)item_off[K] + K));
    hab_agg_plan p;
    if (!hab_agg_make_plan(who, p, item_off, inc ? n_before : nullptr, K)) return 0;
    if (p.n_new && !new_sigs64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const size_t N = p.N, pkb = pk_format ? 64 : 32;
    stage_buf b[] = {{nullptr, results, 4 * K, 64}, {nullptr, out, 32 * (N + K), 64}, {aggsigs_in, nullptr, p.in_bytes, 64}, {pks, nullptr, pkb * N, 64},
                     {msgs32, nullptr, 32 * N, 64}, {new_sigs64, nullptr, 64 * p.n_new, 64}};
    if (!stage_open(e, b, 0, hab_agg_ws(p))) return 0;
    stream_guard sg(e, st);
    return stage_close(e, b, hab_agg_run(e, st, stage_bytes(b), b[0].at<int32_t>(), b[1].at(), b[2].opt(), inc, b[3].at(), pk_format, b[4].at(), b[5].opt(), p));
}
extern "C" int secp256k1_schnorrsig_inc_aggregate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggsigs_out, const unsigned char* aggsigs_in,
                                                            const uint64_t* n_before, const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32,
                                                            const unsigned char* new_sigs64, const uint64_t* item_off, size_t n_aggs) {
    return hab_agg_dev("secp256k1_schnorrsig_inc_aggregate_batch_dev", 1, e, stream, results, aggsigs_out, aggsigs_in, n_before, pubkeys, pk_format, msgs32, new_sigs64, item_off, n_aggs);
}
extern "C" int secp256k1_schnorrsig_inc_aggregate_batch(s2k_engine* e, int32_t* results, unsigned char* aggsigs_out, const unsigned char* aggsigs_in, const uint64_t* n_before,
                                                        const unsigned char* pubkeys, int pk_format, const unsigned char* msgs32, const unsigned char* new_sigs64,
                                                        const uint64_t* item_off, size_t n_aggs) {
    return hab_agg_host("secp256k1_schnorrsig_inc_aggregate_batch", 1, e, results, aggsigs_out, aggsigs_in, n_before, pubkeys, pk_format, msgs32, new_sigs64, item_off, n_aggs);
}
extern "C" int secp256k1_schnorrsig_aggregate_batch_dev(s2k_engine* e, void* stream, int32_t* results, unsigned char* aggsigs_out, const unsigned char* pubkeys, int pk_format,
                                                        const unsigned char* msgs32, const unsigned char* sigs64, const uint64_t* item_off, size_t n_aggs) {
    return hab_agg_dev("secp256k1_schnorrsig_aggregate_batch_dev", 0, e, stream, results, aggsigs_out, nullptr, nullptr, pubkeys, pk_format, msgs32, sigs64, item_off, n_aggs);
}
extern "C" int secp256k1_schnorrsig_aggregate_batch(s2k_engine* e, int32_t* results, unsigned char* aggsigs_out, const unsigned char* pubkeys, int pk_format,
                                                    const unsigned char* msgs32, const unsigned char* sigs64, const uint64_t* item_off, size_t n_aggs) {
    return hab_agg_host("secp256k1_schnorrsig_aggregate_batch", 0, e, results, aggsigs_out, nullptr, nullptr, pubkeys, pk_format, msgs32, sigs64, item_off, n_aggs);
}
