#include "engine_verdict.h"

// ------------------------------------------------------------------------------------------------------------
// one verdict for n BIP-340 signatures (schnorr_all.h): one (2n+1)-term MSM behind a hash tree
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_sa_items(unsigned char* pts, u32* nodes, unsigned char* sc, u32* flags, sa_midstates mid, schnorr_midstate bip340, const unsigned char* sigs,
           const unsigned char* msgs, size_t msglen, const unsigned char* pks, int pk_format, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!sa_item(pts + 128 * i, nodes + 8 * i, sc + 64 * i + 32, mid, bip340, sigs + 64 * i, msgs + msglen * i, msglen, pks + (pk_format ? 64 : 32) * i, pk_format)) flags[0] = 1u;
}
__global__ void k_sa_seed(u32* seed8, unsigned char* seed32_out, sa_midstates mid, const u32* root8, u64 n, u64 msglen) {
    if (threadIdx.x || blockIdx.x) return;
    u32 s[8]; sa_seed(s, mid, root8, n, msglen);
    for (int k = 0; k < 8; k++) seed8[k] = s[k];
    if (seed32_out) sa_words_to_b32(seed32_out, s);
}
__global__ void __launch_bounds__(256)
k_sa_scalars(unsigned char* sc, unsigned char* t, sa_midstates mid, const u32* __restrict__ seed8, const unsigned char* sigs, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 s[8];
    for (int k = 0; k < 8; k++) s[k] = seed8[k];
    sa_scalars(sc + 64 * i, t + 32 * i, mid, s, sigs + 64 * i + 32, i);
}
__global__ void __launch_bounds__(256)
k_sa_sum(unsigned char* out, const unsigned char* __restrict__ in, size_t cnt_in, size_t cnt_out, int negate) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt_out) return;
    const size_t left = cnt_in - SA_FANIN * j;
    sa_sum_node(out + 32 * j, in + 32 * SA_FANIN * j, left < SA_FANIN ? (u32)left : SA_FANIN, negate);
}
// n >= 1
static size_t sa_ws_bytes(const s2k_engine* e, size_t n) {
    const size_t nt = 2 * n + 1;
    return ws_need({128 * n + 64, 64 * n + 64, sa_node_count(n) * 32 + 64, 32 * n + 64, sa_sum_count(n) * 32 + 64, 64, 64}) + msm_ws_bytes(e, nt + 1, engine_msm_plan(e, nt));
}
static const sa_midstates& sa_mid() { static const sa_midstates m = [] { sa_midstates v; sa_make_midstates(v); return v; }(); return m; }
// device pointers in, verdict to d_verdict[0] and (when asked for) the seed to d_seed_out; n >= 1, 2n + 1 <= msm_max_terms.
// Timing: ev[0] .. ev_sa[0] the lift, the item digests and the challenges; .. ev_sa[1] the tree and the seed; .. ev[2] the coefficients, the
// products and the scalar sum; ev[2] .. ev[3] the MSM; ev[1] the end (verdict_tail).
static int sa_launch(s2k_engine* e, hipStream_t st, ws_carver& c, int32_t* d_verdict, unsigned char* d_seed_out, const unsigned char* d_sig, const unsigned char* d_msg,
                     size_t msglen, const unsigned char* d_pk, int pk_format, size_t n) {
    if (!verdict_events(e->ev_sa)) return 0;
    unsigned char* d_pts = c.take<unsigned char>(128 * n + 64); unsigned char* d_sc = c.take<unsigned char>(64 * n + 64);
    u32* d_nodes = c.take<u32>(sa_node_count(n) * 8 + 16); unsigned char* d_t = c.take<unsigned char>(32 * n + 64);
    unsigned char* d_sums = c.take<unsigned char>(sa_sum_count(n) * 32 + 64); u32* d_seed = c.take<u32>(16); u32* d_flags = c.take<u32>(16);
    const sa_midstates& mid = sa_mid();
    HIPCHK(hipMemsetAsync(d_verdict, 0, 4, st));
    HIPCHK(hipMemsetAsync(d_flags, 0, 64, st));
    HIPCHK(hipEventRecord(e->ev[0], st));
    const unsigned bn = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_sa_items, dim3(bn), dim3(256), 0, st, d_pts, d_nodes, d_sc, d_flags, mid, e->bip340, d_sig, d_msg, msglen, d_pk, pk_format, n);
    HIPCHK(hipEventRecord(e->ev_sa[0], st));
    const u32* root = verdict_tree(st, d_nodes, mid, n);
    hipLaunchKernelGGL(k_sa_seed, dim3(1), dim3(64), 0, st, d_seed, d_seed_out, mid, root, (u64)n, (u64)msglen);
    HIPCHK(hipEventRecord(e->ev_sa[1], st));
    hipLaunchKernelGGL(k_sa_scalars, dim3(bn), dim3(256), 0, st, d_sc, d_t, mid, (const u32*)d_seed, d_sig, n);
    // -(sum a_i s_i): the terms, then one level of partial sums per pass; the pass that leaves one value negates it (n = 1: the only pass)
    const unsigned char* in = d_t; unsigned char* out = d_sums;
    size_t cnt = n;
    do {
        const size_t cnt_out = (cnt + SA_FANIN - 1) / SA_FANIN;
        hipLaunchKernelGGL(k_sa_sum, dim3((unsigned)((cnt_out + 255) / 256)), dim3(256), 0, st, out, in, cnt, cnt_out, cnt_out == 1 ? 1 : 0);
        in = out; out += 32 * cnt_out; cnt = cnt_out;
    } while (cnt > 1);
    HIPCHK(hipGetLastError());
    // the MSM's points are R_0, P_0, R_1, P_1, ... with scalars a_0, a_0 e_0, a_1, a_1 e_1, ...; the generator term carries -(sum a_i s_i)
    return verdict_tail(e, st, c, e->ev_sa, d_verdict, d_flags, in, d_sc, d_pts, nullptr, 2 * n);
}
// more than msm_max_terms terms (2n + 1 of them), or more message bytes than a call indexes
static int sa_size_ok(const char* who, const s2k_engine* e, size_t msglen, size_t n) {
    if (n > (msm_max_terms(e) - 1) / 2 || (msglen && n > (size_t(1) << 46) / msglen)) return s2k_fail_arg(who, "batch too large");
    return 1;
}
// every array in HBM; the verdict lands in verdict_dev[0] and the seed, when asked for, in seed32_out_dev (stream-ordered, nothing read back)
extern "C" int secp256k1_schnorrsig_verify_all_dev(s2k_engine* e, void* stream, int32_t* verdict_dev, unsigned char* seed32_out_dev, const unsigned char* sigs,
                                                   const unsigned char* msgs, size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n) {
    if (!e) return s2k_fail("secp256k1_schnorrsig_verify_all_dev", "null engine");
    if (!verdict_dev || pk_format < 0 || pk_format > 1 || ((!sigs || !pubkeys || (!msgs && msglen)) && n))
        return s2k_fail_arg("secp256k1_schnorrsig_verify_all_dev", "illegal argument (ARG_CHECK)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    if (!sa_size_ok("secp256k1_schnorrsig_verify_all_dev", e, msglen, n)) return 0;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    if (n == 0) return verdict_reply(st, verdict_dev, seed32_out_dev, 1u);      // nothing to refuse
    if (!engine_workspace(e, sa_ws_bytes(e, n))) return 0;
    ws_carver c{e->ws, 0};
    return sa_launch(e, st, c, verdict_dev, seed32_out_dev, sigs, msgs, msglen, pubkeys, pk_format, n);
}
// host arrays.  results (n, or NULL): where the verdict is 0 the per-item verifier runs on the buffers already uploaded and says which
// items failed; where it is 1 every item is valid.
extern "C" int secp256k1_schnorrsig_verify_all(s2k_engine* e, int32_t* verdict, int32_t* results, unsigned char* seed32_out, const unsigned char* sigs,
                                               const unsigned char* msgs, size_t msglen, const unsigned char* pubkeys, int pk_format, size_t n) {
    if (!e) return s2k_fail("secp256k1_schnorrsig_verify_all", "null engine");
    if (!verdict || pk_format < 0 || pk_format > 1 || ((!sigs || !pubkeys || (!msgs && msglen)) && n))
        return s2k_fail_arg("secp256k1_schnorrsig_verify_all", "illegal argument (ARG_CHECK)");
    *verdict = 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    if (!sa_size_ok("secp256k1_schnorrsig_verify_all", e, msglen, n)) return 0;
    if (results && n) memset(results, 0, sizeof(int32_t) * n);
    if (seed32_out) memset(seed32_out, 0, 32);
    if (n == 0) { *verdict = 1; return 1; }
    HIPCHK(hipSetDevice(e->device));
    const size_t pkb = pk_format ? 64 : 32;
    const stage_buf in[] = {{sigs, nullptr, 64 * n, 64}, {msgs, nullptr, msglen * n, 64}, {pubkeys, nullptr, pkb * n, 64}};
    return verdict_host(e, in, sa_ws_bytes(e, n), verdict, results, seed32_out, n,
        [&](hipStream_t st, ws_carver& c, int32_t* d_verdict, unsigned char* d_seed, const stage_buf* b) {
            return sa_launch(e, st, c, d_verdict, d_seed, b[0].at(), b[1].at(), msglen, b[2].at(), pk_format, n); },
        // which items: the per-item verifier (it uses the per-lane tables, not the workspace: the uploaded buffers are still there)
        [&](int32_t* d_res, const stage_buf* b) { return secp256k1_schnorrsig_verify_batch_dev(e, nullptr, d_res, b[0].at(), b[1].at(), msglen, b[2].at(), pk_format, n); });
}
// The phases of the most recent verify_all call of this engine, in ms, once its work is complete (s2k_engine_sync): [0] lift, item digests
// and challenges, [1] hash tree and seed, [2] coefficients, products and the scalar sum, [3] the MSM.  -1 where no such call has run.
extern "C" int s2k_schnorr_all_last_split_ms(s2k_engine* e, float* out4) {
    return verdict_split_ms("s2k_schnorr_all_last_split_ms", e, &s2k_engine::ev_sa, out4);
}
