#include "engine_internal.h"
#include "adaptor.h"

// ------------------------------------------------------------------------------------------------------------
// ECDSA adaptor-signature batch verification (adaptor.h) and the two-point multiplication behind its DLEQ half: one item per lane
// ------------------------------------------------------------------------------------------------------------
// Both kernels park a Jacobian point between two multiplications (adaptor.h, ecmult.h: ecmult_lane2_calls).  The parking area lies behind
// the per-lane tables in the engine's table buffer: word k of lane i of a launch of L lanes at park[k * L + i], so a wavefront's store
// or load of one word is 256 contiguous bytes.
static size_t park_lanes(size_t lanes, size_t words) { return (lanes * words + S2K_PTAB_WORDS - 1) / S2K_PTAB_WORDS; }      // the area, counted in table slices

// (no lane leaves early: the to-affine inversion inside adaptor_verify_lane is shared by the 64 lanes of a wavefront)
__global__ void __launch_bounds__(256, 2)
k_adaptor_verify(int32_t* __restrict__ results, const unsigned char* __restrict__ sigs, const unsigned char* __restrict__ pks, const unsigned char* __restrict__ msgs,
                 const unsigned char* __restrict__ eks, int pk_format, adaptor_midstate mid, const u32* __restrict__ gtab, u32* __restrict__ ptab,
                 u32* __restrict__ park, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    const int r = adaptor_verify_lane(mid, sigs, pks, msgs, eks, ii, pk_format, live, gtab, lm, park, i, (size_t)gridDim.x * blockDim.x);
    if (live) results[i] = r;
}

// r = na*A + nb*B: the joint form, the two-call form for a wavefront it declines; to affine and serialised as k_ecmult_batch does
__global__ void __launch_bounds__(256, 2)
k_ecmult2_batch(unsigned char* __restrict__ r_xy, int32_t* __restrict__ r_inf, const unsigned char* __restrict__ a_xy, const unsigned char* __restrict__ a_inf,
                const unsigned char* __restrict__ na, const unsigned char* __restrict__ b_xy, const unsigned char* __restrict__ b_inf,
                const unsigned char* __restrict__ nb, const u32* __restrict__ gtab, u32* __restrict__ ptab, u32* __restrict__ park, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    gej R;
    // term 0: (A, na), term 1: (B, nb); read again from global memory for the two-call form rather than held across the joint form
    auto load = [&](int k, gej& Pj, scalar& sc, size_t at) {
        ge a; ge_load_b64(a, (k ? b_xy : a_xy) + 64 * at); gej_set_ge(Pj, a);
        const unsigned char* inf = k ? b_inf : a_inf;
        Pj.inf = (inf ? (inf[at] != 0) : 0) | !live;
        sc_set_b32(sc, (k ? nb : na) + 32 * at, nullptr);
        if (!live) sc_set_zero(sc);
    };
    int joint;
    {
        gej A, B; scalar sa, sb;
        load(0, A, sa, ii); load(1, B, sb, ii);
        joint = ecmult_lane2(R, A, sa, B, sb, lm);
    }
    if (!joint) {
        const size_t again = ii + s2k_opaque_zero();
        ecmult_lane2_calls(R, [&](int k, gej& Pj, scalar& sc) { load(k, Pj, sc, again); }, gtab, lm, park + (i + s2k_opaque_zero()), (size_t)gridDim.x * blockDim.x);
    }
    ge out;
    ge_set_gej(out, R);
    if (live) {
        if (R.inf) { for (int k = 0; k < 64; k++) r_xy[64 * i + k] = 0; }
        else ge_store_b64(r_xy + 64 * i, out);
        r_inf[i] = R.inf;
    }
}

static int adaptor_format_ok(const char* who, int pk_format) {
    if (pk_format < 0 || pk_format > 2) return s2k_fail_arg(who, "pk_format must be 0 (compressed), 1 (object) or 2 (uncompressed / hybrid)");
    return 1;
}

extern "C" int secp256k1_ecdsa_adaptor_verify_batch_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* adaptor_sigs162,
                                                        const unsigned char* pubkeys, const unsigned char* msgs32, const unsigned char* enckeys, int pk_format, size_t n) {
    const char* who = "secp256k1_ecdsa_adaptor_verify_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !adaptor_sigs162 || !pubkeys || !msgs32 || !enckeys) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (!adaptor_format_ok(who, pk_format)) return 0;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const size_t lanes = ((std::min(n, e->max_lanes) + 255) / 256) * 256;
    if (!engine_ptab(e, lanes + park_lanes(lanes, S2K_ADAPTOR_PARK_WORDS))) return 0;
    u32* const park = e->ptab + lanes * S2K_PTAB_WORDS;
    ENGINE_GTAB(e, st);
    adaptor_midstate mid; adaptor_tag_midstate(mid);                      // (two compressions on the host: not worth a field of the engine)
    HIPCHK(hipMemsetAsync(results, 0, sizeof(int32_t) * n, st));          // a batch that does not complete never shows an item as valid
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);                  // (m <= lanes: every launch's park stride fits the area)
        hipLaunchKernelGGL(k_adaptor_verify, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, results + i0, adaptor_sigs162 + 162 * i0, pubkeys + pkb * i0,
                           msgs32 + 32 * i0, enckeys + pkb * i0, pk_format, mid, e->gtab, e->ptab, park, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int secp256k1_ecdsa_adaptor_verify_batch(s2k_engine* e, int32_t* results, const unsigned char* adaptor_sigs162, const unsigned char* pubkeys,
                                                    const unsigned char* msgs32, const unsigned char* enckeys, int pk_format, size_t n) {
    const char* who = "secp256k1_ecdsa_adaptor_verify_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !adaptor_sigs162 || !pubkeys || !msgs32 || !enckeys) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    memset(results, 0, sizeof(int32_t) * n);
    if (!adaptor_format_ok(who, pk_format)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    if (!engine_workspace(e, ws_need({4 * n, 162 * n, pkb * n, 32 * n, pkb * n}))) return 0;
    ws_carver w{e->ws, 0};
    int32_t* d_res = w.take<int32_t>(n); unsigned char* d_sig = w.take<unsigned char>(162 * n); unsigned char* d_pk = w.take<unsigned char>(pkb * n);
    unsigned char* d_msg = w.take<unsigned char>(32 * n); unsigned char* d_ek = w.take<unsigned char>(pkb * n);
    HIPCHK(hipMemcpyAsync(d_sig, adaptor_sigs162, 162 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_pk, pubkeys, pkb * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_msg, msgs32, 32 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_ek, enckeys, pkb * n, hipMemcpyHostToDevice, e->stream));
    if (!secp256k1_ecdsa_adaptor_verify_batch_dev(e, nullptr, d_res, d_sig, d_pk, d_msg, d_ek, pk_format, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(results, d_res, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

extern "C" int s2k_ecmult2_batch_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                                     const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n) {
    const char* who = "s2k_ecmult2_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!r_xy || !r_inf || !a_xy || !na || !b_xy || !nb) return s2k_fail_arg(who, "illegal argument (a NULL array)");
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    const size_t lanes = ((std::min(n, e->max_lanes) + 255) / 256) * 256;
    if (!engine_ptab(e, lanes + park_lanes(lanes, S2K_PARK_GEJ_WORDS))) return 0;
    u32* const park = e->ptab + lanes * S2K_PTAB_WORDS;
    ENGINE_GTAB(e, st);
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);
        hipLaunchKernelGGL(k_ecmult2_batch, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, r_xy + 64 * i0, r_inf + i0, a_xy + 64 * i0, a_inf ? a_inf + i0 : nullptr,
                           na + 32 * i0, b_xy + 64 * i0, b_inf ? b_inf + i0 : nullptr, nb + 32 * i0, e->gtab, e->ptab, park, m);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}
extern "C" int s2k_ecmult2_batch(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                                 const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n) {
    const char* who = "s2k_ecmult2_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!r_xy || !r_inf || !a_xy || !na || !b_xy || !nb) return s2k_fail_arg(who, "illegal argument (a NULL array)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    if (!engine_workspace(e, ws_need({64 * n, 4 * n, 64 * n, n, 32 * n, 64 * n, n, 32 * n}))) return 0;
    ws_carver w{e->ws, 0};
    unsigned char* d_r = w.take<unsigned char>(64 * n); int32_t* d_inf = w.take<int32_t>(n);
    unsigned char* d_a = w.take<unsigned char>(64 * n); unsigned char* d_ai = w.take<unsigned char>(n); unsigned char* d_na = w.take<unsigned char>(32 * n);
    unsigned char* d_b = w.take<unsigned char>(64 * n); unsigned char* d_bi = w.take<unsigned char>(n); unsigned char* d_nb = w.take<unsigned char>(32 * n);
    HIPCHK(hipMemcpyAsync(d_a, a_xy, 64 * n, hipMemcpyHostToDevice, e->stream));
    if (a_inf) HIPCHK(hipMemcpyAsync(d_ai, a_inf, n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_na, na, 32 * n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_b, b_xy, 64 * n, hipMemcpyHostToDevice, e->stream));
    if (b_inf) HIPCHK(hipMemcpyAsync(d_bi, b_inf, n, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_nb, nb, 32 * n, hipMemcpyHostToDevice, e->stream));
    if (!s2k_ecmult2_batch_dev(e, nullptr, d_r, d_inf, d_a, a_inf ? d_ai : nullptr, d_na, d_b, b_inf ? d_bi : nullptr, d_nb, n)) { (void)hipStreamSynchronize(e->stream); return 0; }
    HIPCHK(hipMemcpyAsync(r_xy, d_r, 64 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(r_inf, d_inf, 4 * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}
