#include "engine_lanes.h"
#include "whitelist.h"

// ------------------------------------------------------------------------------------------------------------
// Whitelist-signature batch verification (whitelist.h): k_wl_keys one lane per (item, key) pair, k_wl_ring one lane per item
// ------------------------------------------------------------------------------------------------------------
// The plan, built on the host from the caller's offset arrays (wl_impl):
//   key_off[n + 1]   prefix sums of the items' key-lane counts: the list's length for an item that runs (wl_item_planned), 0 for one
//                    that does not -- such an item takes no lane of k_wl_keys; pair p belongs to the item i with key_off[i] <= p < key_off[i + 1]
//   item_list[n]     the item's list
//   list_off[L + 1], sig_off[n + 1]   the caller's arrays
struct wl_plan_dev { const uint64_t* key_off; const u32* item_list; const uint64_t* list_off; const uint64_t* sig_off; };

// (no lane leaves early in either kernel: the to-affine inversions are shared by the 64 lanes of a wavefront)
__global__ void __launch_bounds__(256, 2)
k_wl_keys(u32* __restrict__ keys28, wl_plan_dev P, const unsigned char* __restrict__ online64, const unsigned char* __restrict__ offline64,
          const unsigned char* __restrict__ sub64, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t p0, size_t m, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = t < m;
    const uint64_t p = p0 + (live ? t : 0);
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + t * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    size_t lo = 0, hi = n;                                        // the last i with key_off[i] <= p  (key_off[0] = 0 <= p < key_off[n])
    while (hi - lo > 1) { const size_t mid = lo + (hi - lo) / 2; if (P.key_off[mid] <= p) lo = mid; else hi = mid; }
    const uint64_t k = P.list_off[P.item_list[lo]] + (p - P.key_off[lo]);
    wl_key_lane(keys28 + WL_KEY_WORDS * p, online64 + 64 * k, offline64 + 64 * k, sub64 + 64 * lo, live, gtab, lm);
}
__global__ void __launch_bounds__(256, 2)
k_wl_ring(int32_t* __restrict__ results, const u32* __restrict__ keys28, u32* __restrict__ msg8, wl_plan_dev P, const unsigned char* __restrict__ sigs,
          const unsigned char* __restrict__ online64, const unsigned char* __restrict__ offline64, const unsigned char* __restrict__ sub64,
          const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t i0, size_t m) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = t < m;
    const size_t i = i0 + (live ? t : 0);
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + t * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const u32 l = P.item_list[i];
    const uint64_t k0 = P.list_off[l], nk = P.list_off[l + 1] - k0, s0 = P.sig_off[i], s1 = P.sig_off[i + 1];
    const int r = wl_ring_lane(sigs + s0, s1 - s0, keys28 + WL_KEY_WORDS * P.key_off[i], online64 + 64 * k0, offline64 + 64 * k0, nk, sub64 + 64 * i,
                               msg8 + 8 * i, live, gtab, lm);
    if (live) results[i] = r;
}

// The three host arrays as the caller gave them: 0 and S2K_STATUS_ILLEGAL_ARGUMENT where they do not describe a batch.
static int wl_check(const char* who, const uint64_t* sig_off, const uint64_t* list_off, size_t n_lists, const u32* list_of, size_t n) {
    if (!list_of && n_lists != n) return s2k_fail_arg(who, "list_of == NULL needs n_lists == n");
    if (list_off[0] != 0) return s2k_fail_arg(who, "list_off must start at 0");
    for (size_t l = 0; l < n_lists; l++) if (list_off[l + 1] < list_off[l]) return s2k_fail_arg(who, "list_off must not decrease");
    for (size_t i = 0; i < n; i++) if (sig_off[i + 1] < sig_off[i]) return s2k_fail_arg(who, "sig_off must not decrease");
    if (list_of) for (size_t i = 0; i < n; i++) if (list_of[i] >= n_lists) return s2k_fail_arg(who, "list_of names a list that is not there");
    return 1;
}
static size_t wl_pairs(const uint64_t* sig_off, const uint64_t* list_off, const u32* list_of, size_t n) {
    size_t pairs = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t l = list_of ? list_of[i] : i;
        const uint64_t nk = list_off[l + 1] - list_off[l];
        if (wl_item_planned(nk, sig_off[i + 1] - sig_off[i])) pairs += (size_t)nk;
    }
    return pairs;
}
static size_t wl_ws_bytes(size_t n, size_t n_lists, size_t pairs) {
    return ws_need({8 * (n + 1), 4 * n + 64, 8 * (n_lists + 1), 8 * (n + 1), 32 * n + 64, 4 * WL_KEY_WORDS * pairs + 64});
}
// Every byte array in HBM, the offset / index arrays on the host (already checked; sig_off relative to `sigs`).  The workspace from
// `front` on is this function's; the caller has sized it (wl_ws_bytes).
static int wl_impl(s2k_engine* e, hipStream_t st, size_t front, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                   const unsigned char* online64, const unsigned char* offline64, const uint64_t* list_off, size_t n_lists, const u32* list_of,
                   const unsigned char* sub64, size_t n) {
    std::vector<uint64_t> key_off(n + 1);
    std::vector<u32> item_list(n);
    key_off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t l = list_of ? list_of[i] : i;
        const uint64_t nk = list_off[l + 1] - list_off[l];
        item_list[i] = (u32)l;
        key_off[i + 1] = key_off[i] + (wl_item_planned(nk, sig_off[i + 1] - sig_off[i]) ? nk : 0);
    }
    const size_t pairs = (size_t)key_off[n];
    if (!engine_ptab(e, ((std::min(std::max(n, pairs), e->max_lanes) + 255) / 256) * 256)) return 0;
    ENGINE_GTAB(e, st);
    ws_carver c{e->ws, front};
    uint64_t* d_key_off = c.take<uint64_t>(n + 1); u32* d_item_list = c.take<u32>(n + 16); uint64_t* d_list_off = c.take<uint64_t>(n_lists + 1);
    uint64_t* d_sig_off = c.take<uint64_t>(n + 1); u32* d_msg = c.take<u32>(8 * n + 16); u32* d_keys = c.take<u32>(WL_KEY_WORDS * pairs + 16);
    HIPCHK(hipMemcpyAsync(d_key_off, key_off.data(), 8 * (n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_item_list, item_list.data(), 4 * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_list_off, list_off, 8 * (n_lists + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_sig_off, sig_off, 8 * (n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(e->ev_fork, st));                     // (the host arrays must have been consumed before the call returns)
    const wl_plan_dev P{d_key_off, d_item_list, d_list_off, d_sig_off};
    HIPCHK(hipEventRecord(e->ev[0], st));
    for (size_t p0 = 0; p0 < pairs; p0 += e->max_lanes) {
        const size_t m = std::min(pairs - p0, e->max_lanes);
        hipLaunchKernelGGL(k_wl_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_keys, P, online64, offline64, sub64, e->gtab, e->ptab, p0, m, n);
    }
    HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_wl_ring, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results, (const u32*)d_keys, d_msg, P, sigs, online64, offline64, sub64,
                           e->gtab, e->ptab, i0, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    HIPCHK(hipEventSynchronize(e->ev_fork));
    return 1;
}

extern "C" int secp256k1_whitelist_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off_host,
                                                    const unsigned char* online64, const unsigned char* offline64, const uint64_t* list_off_host, size_t n_lists,
                                                    const uint32_t* list_of_host, const unsigned char* sub64, size_t n) {
    const char* who = "secp256k1_whitelist_verify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !sig_off_host || !online64 || !offline64 || !list_off_host || !sub64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete never shows an item as valid
    if (!wl_check(who, sig_off_host, list_off_host, n_lists, list_of_host, n)) return 0;
    if (!engine_workspace(e, wl_ws_bytes(n, n_lists, wl_pairs(sig_off_host, list_off_host, list_of_host, n)))) return 0;
    return wl_impl(e, st, 0, results, sigs, sig_off_host, online64, offline64, list_off_host, n_lists, list_of_host, sub64, n);
}
extern "C" int secp256k1_whitelist_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* sigs, const uint64_t* sig_off,
                                                const unsigned char* online64, const unsigned char* offline64, const uint64_t* list_off, size_t n_lists,
                                                const uint32_t* list_of, const unsigned char* sub64, size_t n) {
    const char* who = "secp256k1_whitelist_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !sig_off || !online64 || !offline64 || !list_off || !sub64) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (!wl_check(who, sig_off, list_off, n_lists, list_of, n)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    // the items' bytes [sig_off[0], sig_off[n]) go to HBM as they are, with offsets relative to their start; every list is uploaded once
    const size_t sig_lo = (size_t)sig_off[0], sig_bytes = (size_t)(sig_off[n] - sig_off[0]), key_bytes = 64 * (size_t)list_off[n_lists];
    hipStream_t st = e->stream;
    stage_buf b[] = {{nullptr, results, 4 * n}, {sigs + sig_lo, nullptr, sig_bytes, 64}, {online64, nullptr, key_bytes, 64}, {offline64, nullptr, key_bytes, 64}, {sub64, nullptr, 64 * n}};
    if (!stage_open(e, b, 0, wl_ws_bytes(n, n_lists, wl_pairs(sig_off, list_off, list_of, n)))) return 0;
    stream_guard sg(e, st);
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = sig_off[i] - sig_lo;
    HIPCHK(hipMemsetAsync(b[0].dev, 0, sizeof(int32_t) * n, st));
    return stage_close(e, b, wl_impl(e, st, stage_bytes(b), b[0].at<int32_t>(), b[1].at(), rel.data(), b[2].at(), b[3].at(), list_off, n_lists, list_of, b[4].at(), n));
}
