#include "engine_lanes.h"
#include "adaptor.h"

// ------------------------------------------------------------------------------------------------------------
// ECDSA adaptor-signature batch verification (adaptor.h) and the two-point multiplication behind its DLEQ half: one item per lane
// ------------------------------------------------------------------------------------------------------------
// Both kernels park a Jacobian point between two multiplications (adaptor.h, ecmult.h: ecmult_lane2_calls), in the parking area behind
// the per-lane tables (engine_lanes.h: park_lanes).

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
    adaptor_midstate mid; adaptor_tag_midstate(mid);                      // (two compressions on the host: not worth a field of the engine)
    const size_t pkb = ecdsa_pk_bytes(pk_format);
    return lanes_run(e, stream, n, {true, true, S2K_ADAPTOR_PARK_WORDS}, {{results, sizeof(int32_t) * n}},      // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32* park) {
        hipLaunchKernelGGL(k_adaptor_verify, grid, dim3(256), 0, st, results + i0, adaptor_sigs162 + 162 * i0, pubkeys + pkb * i0, msgs32 + 32 * i0, enckeys + pkb * i0,
                           pk_format, mid, e->gtab, e->ptab, park, m);
    });
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
    stage_buf b[] = {{nullptr, results, 4 * n}, {adaptor_sigs162, nullptr, 162 * n}, {pubkeys, nullptr, pkb * n}, {msgs32, nullptr, 32 * n}, {enckeys, nullptr, pkb * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_ecdsa_adaptor_verify_batch_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].at(), b[4].at(), pk_format, n));
}

extern "C" int s2k_ecmult2_batch_dev(s2k_engine* e, void* stream, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                                     const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n) {
    const char* who = "s2k_ecmult2_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!r_xy || !r_inf || !a_xy || !na || !b_xy || !nb) return s2k_fail_arg(who, "illegal argument (a NULL array)");
    return lanes_run(e, stream, n, {true, true, S2K_PARK_GEJ_WORDS}, {}, [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32* park) {
        hipLaunchKernelGGL(k_ecmult2_batch, grid, dim3(256), 0, st, r_xy + 64 * i0, r_inf + i0, a_xy + 64 * i0, a_inf ? a_inf + i0 : nullptr, na + 32 * i0, b_xy + 64 * i0,
                           b_inf ? b_inf + i0 : nullptr, nb + 32 * i0, e->gtab, e->ptab, park, m);
    });
}
extern "C" int s2k_ecmult2_batch(s2k_engine* e, unsigned char* r_xy, int32_t* r_inf, const unsigned char* a_xy, const unsigned char* a_inf,
                                 const unsigned char* na, const unsigned char* b_xy, const unsigned char* b_inf, const unsigned char* nb, size_t n) {
    const char* who = "s2k_ecmult2_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!r_xy || !r_inf || !a_xy || !na || !b_xy || !nb) return s2k_fail_arg(who, "illegal argument (a NULL array)");
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, r_xy, 64 * n}, {nullptr, r_inf, 4 * n}, {a_xy, nullptr, 64 * n}, {a_inf, nullptr, n}, {na, nullptr, 32 * n},
                     {b_xy, nullptr, 64 * n}, {b_inf, nullptr, n}, {nb, nullptr, 32 * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, s2k_ecmult2_batch_dev(e, nullptr, b[0].at(), b[1].at<int32_t>(), b[2].at(), b[3].opt(), b[4].at(), b[5].at(), b[6].opt(), b[7].at(), n));
}
