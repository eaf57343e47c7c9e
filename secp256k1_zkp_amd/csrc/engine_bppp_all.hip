#include "engine_verdict.h"
#include "bppp_all.h"

// ------------------------------------------------------------------------------------------------------------
// one verdict for n BP++ norm arguments over one generator set (bppp_all.h): one (n_gens + 1 + n (2 n_rounds + 1))-term MSM behind a hash tree
// ------------------------------------------------------------------------------------------------------------
// the sum's points are  generators 0 .. n_gens - 1, then the own terms of proof 0, of proof 1, ...: lane t parses point t (a square root each)
__global__ void __launch_bounds__(256)
k_ba_points(unsigned char* pts, unsigned char* inf, u32* flags, const unsigned char* gens33, u32 n_gens, u32 own, const unsigned char* proofs, size_t proof_len,
            const unsigned char* commits33, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int ok = 1;
    if (t < n_gens) ok = ba_gen(pts + 64 * t, inf + t, gens33 + 33 * t);
    else {
        const size_t q = t - n_gens, p = q / own;
        if (p >= n) return;
        ok = ba_own_point(pts + 64 * t, inf + t, (u32)(q % own), proofs + p * proof_len, commits33 + 33 * p);
    }
    if (!ok) flags[0] = 1u;
}
__global__ void __launch_bounds__(64)
k_ba_proofs(u32* term_sc, u32* sg_factors, u32* nodes, int* proof_ok, u32* flags, sa_midstates mid, bp_shape sh, const unsigned char* proofs, size_t proof_len,
            const unsigned char* transcripts, const unsigned char* rho, const unsigned char* c_vec, const unsigned char* commits33, size_t n) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int ok = ba_proof(term_sc + p * sh.n_terms * 8, sg_factors + p * (8 * BP_MAX_LOG_G), nodes + 8 * p, mid, sh, proofs + p * proof_len, proof_len,
                            transcripts + 104 * p, rho + 32 * p, c_vec + p * sh.h_len * 32, commits33 + 33 * p);
    proof_ok[p] = ok;
    if (!ok) flags[0] = 1u;
}
__global__ void __launch_bounds__(256)
k_ba_sg(u32* term_sc, const u32* sg_factors, const int* proof_ok, bp_shape sh, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p = t / (sh.g_len - 1); const u32 i = 1u + (u32)(t % (sh.g_len - 1));
    if (p >= n || !proof_ok[p]) return;
    bp_sg_entry(term_sc + p * sh.n_terms * 8, sg_factors + p * (8 * BP_MAX_LOG_G), sh, i);
}
struct ba_gd { u32 w[8]; };
__global__ void k_ba_seed(u32* seed8, unsigned char* seed32_out, sa_midstates mid, ba_gd gd, const u32* root8, u64 n, u64 proof_len, u64 h_len) {
    if (threadIdx.x || blockIdx.x) return;
    u32 s[8]; ba_seed(s, mid, gd.w, root8, n, proof_len, h_len);
    for (int k = 0; k < 8; k++) seed8[k] = s[k];
    if (seed32_out) sa_words_to_b32(seed32_out, s);
}
__global__ void __launch_bounds__(256)
k_ba_coeff(u32* zp, sa_midstates mid, const u32* __restrict__ seed8, size_t n) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    u32 s[8];
    for (int k = 0; k < 8; k++) s[k] = seed8[k];
    ba_coeff(zp + 8 * p, mid, s, p);
}
// lane = chunk * ncols + col: adjacent lanes take adjacent columns, so a wavefront's loads of sc[p][.] are one contiguous run and z'_p is
// one address for (almost) the whole wavefront
__global__ void __launch_bounds__(256)
k_ba_colsum(u32* out, const u32* __restrict__ term_sc, const u32* __restrict__ zp, u32 n_terms, u32 ncols, u32 chunk_len, size_t chunks, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t ch = t / ncols; const u32 col = (u32)(t % ncols);
    if (ch >= chunks) return;
    const size_t p0 = ch * chunk_len, p1 = p0 + chunk_len < n ? p0 + chunk_len : n;
    ba_colsum(out + t * 8, term_sc, zp, n_terms, col, p0, p1);
}
// last pass (cnt_out == 1, last != 0): column col < ncols - 1 is the scalar of generator col, the last column the scalar of G
__global__ void __launch_bounds__(256)
k_ba_colsum_node(u32* out, unsigned char* sc_out, unsigned char* g_out, const u32* __restrict__ in, u32 ncols, size_t cnt_in, size_t cnt_out, int last) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t j = t / ncols; const u32 col = (u32)(t % ncols);
    if (j >= cnt_out) return;
    const size_t left = cnt_in - SA_FANIN * j;
    ba_colsum_node(out + t * 8, last ? (col + 1 < ncols ? sc_out + 32 * (size_t)col : g_out) : nullptr, in + (size_t)SA_FANIN * j * ncols * 8, ncols, col,
                   left < SA_FANIN ? (u32)left : SA_FANIN);
}
__global__ void __launch_bounds__(256)
k_ba_own_scalars(unsigned char* sc, bp_shape sh, u32 own, const u32* __restrict__ term_sc, const u32* __restrict__ zp, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p = t / own;
    if (p >= n) return;
    ba_own_scalar(sc + 32 * ((size_t)sh.n_gens + t), sh, (u32)(t % own), term_sc + p * sh.n_terms * 8, zp + 8 * p);
}
static size_t ba_own_terms(const bp_shape& sh) { return 2 * (size_t)sh.n_rounds + 1; }
static size_t ba_msm_points(const bp_shape& sh, size_t n) { return (size_t)sh.n_gens + n * ba_own_terms(sh); }
// n >= 1
static size_t ba_ws_bytes(const s2k_engine* e, const bp_shape& sh, size_t n) {
    const size_t M = ba_msm_points(sh, n), nt = M + 1, ncols = (size_t)sh.n_gens + 1;
    return ws_need({n * sh.n_terms * 32, n * 32 * BP_MAX_LOG_G, sa_node_count(n) * 32 + 64, 4 * n + 64, 32 * n + 64, ba_colsum_rows(n) * ncols * 32 + 64, 64 * M + 64, M + 64,
                    32 * M + 64, 64, 64, 64}) + msm_ws_bytes(e, nt + 1, engine_msm_plan(e, nt));
}
static const sa_midstates& ba_mid() { static const sa_midstates m = [] { sa_midstates v; ba_make_midstates(v); return v; }(); return m; }
// device pointers in, verdict to d_verdict[0] and (when asked for) the seed to d_seed_out; n >= 1, a shape bp_make_shape accepts with log_g <= BP_MAX_LOG_G,
// n_gens + n (2 n_rounds + 1) <= msm_max_terms.
// Timing: ev[0] .. ev_ba[0] the per-proof scalars and the item digests; .. ev_ba[1] the tree, the seed and z'; .. ev[2] the column sums,
// the own terms' scalars and whatever is left of the points on the side stream; ev[2] .. ev[3] the MSM; ev[1] the end (verdict_tail).
static int ba_launch(s2k_engine* e, hipStream_t st, ws_carver& c, int32_t* d_verdict, unsigned char* d_seed_out, const bp_shape& sh, const unsigned char* d_pr, size_t proof_len,
                     const unsigned char* d_tr, const unsigned char* d_rho, const unsigned char* d_g33, const unsigned char* gens33_host, const unsigned char* d_cv,
                     const unsigned char* d_cm, size_t n) {
    if (!verdict_events(e->ev_ba)) return 0;
    const size_t own = ba_own_terms(sh), M = ba_msm_points(sh, n);
    const u32 ncols = sh.n_gens + 1u;
    size_t ccounts[SA_MAX_LEVELS]; u32 chunk_len;
    const int cpasses = ba_colsum_plan(ccounts, &chunk_len, n);
    u32* term_sc = c.take<u32>(n * sh.n_terms * 8); u32* sg_factors = c.take<u32>(n * 8 * BP_MAX_LOG_G);
    u32* d_nodes = c.take<u32>(sa_node_count(n) * 8 + 16); int* proof_ok = c.take<int>(n + 16); u32* d_zp = c.take<u32>(8 * n + 16);
    u32* d_part = c.take<u32>(ba_colsum_rows(n) * ncols * 8 + 16);
    unsigned char* d_pts = c.take<unsigned char>(64 * M + 64); unsigned char* d_inf = c.take<unsigned char>(M + 64); unsigned char* d_sc = c.take<unsigned char>(32 * M + 64);
    unsigned char* d_gsc = c.take<unsigned char>(64); u32* d_seed = c.take<u32>(16); u32* d_flags = c.take<u32>(16);
    const sa_midstates& mid = ba_mid();
    ba_gd gd; ba_gens_digest(gd.w, gens33_host, sh.n_gens, sh.g_len);
    HIPCHK(hipMemsetAsync(d_verdict, 0, 4, st));
    HIPCHK(hipMemsetAsync(d_flags, 0, 64, st));
    HIPCHK(hipEventRecord(e->ev[0], st));
    // the points need nothing but the inputs, and each is a square root (a third of a millisecond of latency whatever the batch size): they are
    // parsed on the side stream underneath the per-proof lanes, the tree and the column sums, which leave most of the machine idle
    HIPCHK(hipEventRecord(e->ev_msm_fork, st));
    HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_msm_fork, 0));
    hipLaunchKernelGGL(k_ba_points, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, e->stream2, d_pts, d_inf, d_flags, d_g33, sh.n_gens, (u32)own, d_pr, proof_len, d_cm, n);
    HIPCHK(hipEventRecord(e->ev_msm_join, e->stream2));
    hipLaunchKernelGGL(k_ba_proofs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, term_sc, sg_factors, d_nodes, proof_ok, d_flags, mid, sh, d_pr, proof_len, d_tr, d_rho, d_cv, d_cm, n);
    if (sh.g_len > 1) hipLaunchKernelGGL(k_ba_sg, dim3((unsigned)((n * (sh.g_len - 1) + 255) / 256)), dim3(256), 0, st, term_sc, (const u32*)sg_factors, (const int*)proof_ok, sh, n);
    HIPCHK(hipEventRecord(e->ev_ba[0], st));
    const u32* root = verdict_tree(st, d_nodes, mid, n);
    hipLaunchKernelGGL(k_ba_seed, dim3(1), dim3(64), 0, st, d_seed, d_seed_out, mid, gd, root, (u64)n, (u64)proof_len, (u64)sh.h_len);
    hipLaunchKernelGGL(k_ba_coeff, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_zp, mid, (const u32*)d_seed, n);
    HIPCHK(hipEventRecord(e->ev_ba[1], st));
    // S_t and g_sc: one pass over chunks of proofs, then partial sums with fan-in 16; the pass that leaves one row writes the sum's scalars
    hipLaunchKernelGGL(k_ba_colsum, dim3((unsigned)((ccounts[0] * ncols + 255) / 256)), dim3(256), 0, st, d_part, (const u32*)term_sc, (const u32*)d_zp, sh.n_terms, ncols, chunk_len, ccounts[0], n);
    {
        const u32* in = d_part;
        for (int k = 0; k + 1 < cpasses; k++) {
            const int last = (k + 2 == cpasses);
            u32* out = const_cast<u32*>(in) + ccounts[k] * ncols * 8;                // (the last pass writes no words: it has no row of its own)
            hipLaunchKernelGGL(k_ba_colsum_node, dim3((unsigned)((ccounts[k + 1] * ncols + 255) / 256)), dim3(256), 0, st, out, d_sc, d_gsc, in, ncols, ccounts[k], ccounts[k + 1], last);
            in = out;
        }
    }
    hipLaunchKernelGGL(k_ba_own_scalars, dim3((unsigned)((n * own + 255) / 256)), dim3(256), 0, st, d_sc, sh, (u32)own, (const u32*)term_sc, (const u32*)d_zp, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamWaitEvent(st, e->ev_msm_join, 0));
    return verdict_tail(e, st, c, e->ev_ba, d_verdict, d_flags, d_gsc, d_sc, d_pts, d_inf, M);
}
// more points than one sum indexes, or more bytes than a call indexes
static int ba_size_ok(const char* who, const s2k_engine* e, const bp_shape& sh, size_t n) {
    const size_t cap = msm_max_terms(e);
    if (sh.n_gens >= cap || n > (cap - 1 - sh.n_gens) / ba_own_terms(sh) || n > (size_t(1) << 46) / ((size_t)sh.n_terms * 32)) return s2k_fail_arg(who, "batch too large");
    return 1;
}
// every array in HBM; the verdict lands in verdict_dev[0] and the seed, when asked for, in seed32_out_dev (stream-ordered, nothing read back)
extern "C" int secp256k1_bppp_norm_product_verify_all_dev(s2k_engine* e, void* stream, int32_t* verdict_dev, unsigned char* seed32_out_dev, const unsigned char* proofs,
                                                          size_t proof_len, const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33_dev,
                                                          const unsigned char* gens33_host, size_t n_gens, size_t g_len, const unsigned char* c_vec, size_t c_vec_len,
                                                          const unsigned char* commits33, size_t n) {
    static const char who[] = "secp256k1_bppp_norm_product_verify_all_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (!verdict_dev || ((!proofs || !transcripts || !rho || !gens33_dev || !gens33_host || !c_vec || !commits33) && n)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    bp_shape sh;
    const int shape_ok = n ? bp_make_shape(sh, g_len, c_vec_len, n_gens, proof_len) : 0;
    if (shape_ok && sh.log_g > BP_MAX_LOG_G) return s2k_fail(who, "g_len above 256 is not supported by this engine");
    if (shape_ok && !ba_size_ok(who, e, sh, n)) return 0;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (!shape_ok) return verdict_reply(st, verdict_dev, seed32_out_dev, n ? 0u : 1u);      // n == 0: nothing to refuse; a shape the reference refuses (:446-461): verdict 0
    if (!engine_workspace(e, ba_ws_bytes(e, sh, n))) return 0;
    ws_carver c{e->ws, 0};
    return ba_launch(e, st, c, verdict_dev, seed32_out_dev, sh, proofs, proof_len, transcripts, rho, gens33_dev, gens33_host, c_vec, commits33, n);
}
// host arrays.  results (n, or NULL): where the verdict is 0 the per-item verifier runs on the buffers already uploaded and says which
// proofs failed; where it is 1 every proof is valid.
extern "C" int secp256k1_bppp_norm_product_verify_all(s2k_engine* e, int32_t* verdict, int32_t* results, unsigned char* seed32_out, const unsigned char* proofs,
                                                      size_t proof_len, const unsigned char* transcripts, const unsigned char* rho, const unsigned char* gens33,
                                                      size_t n_gens, size_t g_len, const unsigned char* c_vec, size_t c_vec_len, const unsigned char* commits33, size_t n) {
    static const char who[] = "secp256k1_bppp_norm_product_verify_all";
    if (!e) return s2k_fail(who, "null engine");
    if (!verdict || ((!proofs || !transcripts || !rho || !gens33 || !c_vec || !commits33) && n)) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    *verdict = 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    bp_shape sh;
    const int shape_ok = n ? bp_make_shape(sh, g_len, c_vec_len, n_gens, proof_len) : 0;
    if (shape_ok && sh.log_g > BP_MAX_LOG_G) return s2k_fail(who, "g_len above 256 is not supported by this engine");
    if (shape_ok && !ba_size_ok(who, e, sh, n)) return 0;
    if (results && n) memset(results, 0, sizeof(int32_t) * n);
    if (seed32_out) memset(seed32_out, 0, 32);
    if (n == 0) { *verdict = 1; return 1; }
    if (!shape_ok) return 1;                                   // :446-461: every proof refused
    HIPCHK(hipSetDevice(e->device));
    // The locating call carves the workspace from offset 0 and may grow it: sized once, for the larger of the two front parts, with the
    // uploads behind both, so that it neither reallocates nor overwrites them.
    const size_t per = std::max<size_t>(1, e->max_lanes / sh.n_terms);
    const size_t front = std::max(ba_ws_bytes(e, sh, n), results ? bpv_ws_bytes(std::min(n, per), sh) : (size_t)0);
    const stage_buf in[] = {{proofs, nullptr, n * proof_len, 64}, {transcripts, nullptr, 104 * n}, {rho, nullptr, 32 * n}, {gens33, nullptr, 33 * n_gens},
                            {c_vec, nullptr, 32 * c_vec_len * n}, {commits33, nullptr, 33 * n}};
    return verdict_host(e, in, front, verdict, results, seed32_out, n,
        [&](hipStream_t st, ws_carver& c, int32_t* d_verdict, unsigned char* d_seed, const stage_buf* b) {
            return ba_launch(e, st, c, d_verdict, d_seed, sh, b[0].at(), proof_len, b[1].at(), b[2].at(), b[3].at(), gens33, b[4].at(), b[5].at(), n); },
        [&](int32_t* d_res, const stage_buf* b) {
            return secp256k1_bppp_norm_product_verify_batch_dev(e, nullptr, d_res, b[0].at(), proof_len, b[1].at(), b[2].at(), b[3].at(), gens33, n_gens, g_len, b[4].at(), c_vec_len,
                                                                b[5].at(), n); });
}
// The phases of the most recent verify_all call of this engine, in ms, once its work is complete (s2k_engine_sync): [0] generators, per-proof
// scalars and item digests, [1] hash tree, seed and z', [2] column sums and own terms, [3] the MSM.  -1 where no such call has run.
extern "C" int s2k_bppp_all_last_split_ms(s2k_engine* e, float* out4) {
    return verdict_split_ms("s2k_bppp_all_last_split_ms", e, &s2k_engine::ev_ba, out4);
}
