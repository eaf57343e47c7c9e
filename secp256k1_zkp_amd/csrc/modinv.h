// modinv.h -- inverse modulo the field prime p and the group order n by division steps, organised for a 64-lane wavefront.
//
// Role of the reference's secp256k1_fe_inv_var / secp256k1_scalar_inverse_var (src/field_5x52_impl.h:491-522,
// src/scalar_4x64_impl.h, both on src/modinv64_impl.h).  The algorithm is Bernstein-Yang "safegcd" in the half-delta form
// whose iteration bound the reference's doc/safegcd_implementation.md (sections 1-5) derives: starting from delta = 1/2,
// 590 division steps bring any g below a 256-bit odd modulus f to 0; 20 batches of 30 are run.  The *organisation* is this
// engine's own:
//
//  * Batch kernel (`ds_batch`): the 30 steps of a batch only look at the low 32 bits of f and g.  A lane does not walk them one
//    by one: every loop trip first retires the whole run of even-g steps at once (one count-trailing-zeros, three variable
//    shifts) and then one odd-g step written with selects, so a trip advances a lane by 2 steps on average.  The trip loop is
//    closed by a wavefront vote -- it runs until the slowest lane has used its 30 steps (typically 18-21 trips), lanes that are
//    done ride along with all updates predicated off.  No lane ever branches on its data.
//  * Transition matrices are applied to (f, g) exactly and to (d, e) modulo m with 32x32+64 signed multiply-accumulates
//    (v_mad_i64_i32), nine 30-bit limbs per operand.  (d, e) are NOT renormalised per batch: each batch adds a multiple
//    k*m, 0 <= k < 2^30, chosen to clear the low 30 bits, which lets |d|, |e| grow by at most m per batch -- 21 m < 2^261
//    after 20 batches, well inside the 270-bit signed limbs -- and one short reduction at the very end (quotient estimate
//    from the top limb, one multiply-subtract, one conditional subtraction) brings the result to [0, m).
//
// Everything is branch-free per lane and the same for both moduli; the modulus is a compile-time constant, so p's zero limbs
// cost nothing.  Result: a^-1 mod m, and 0 for a = 0.
#pragma once
#include "s2k_common.h"

#define DS_LIMBS 9
#define DS_BITS 30
#define DS_MASK ((int32_t)0x3FFFFFFF)
#define DS_BATCHES 20

struct ds_int { int32_t w[DS_LIMBS]; };                 // value = sum w[i] 2^(30 i); w[0..7] in [0, 2^30), w[8] signed
struct ds_modulus { int32_t w[DS_LIMBS]; u32 inv; };    // modulus in that form (limbs may be negative: a sparse signed form), m^-1 mod 2^30

// p = 2^256 - 2^32 - 977 = 65536 * 2^240 - 4 * 2^30 - 977
#define DS_MOD_P ds_modulus{{-977, -4, 0, 0, 0, 0, 0, 0, 65536}, 0x2DDACACFu}
// n = group order of secp256k1
#define DS_MOD_N ds_modulus{{0x10364141, 0x3F497A33, 0x348A03BB, 0x2BB739AB, 0x3FFFFEBA, 0x3FFFFFFF, 0x3FFFFFFF, 0x3FFFFFFF, 0xFFFF}, 0x2A774EC1u}

#if defined(__HIP_DEVICE_COMPILE__)
#define DS_WAVE_ANY(p) (__any(p))
#define DS_WAVE_ALL(p) (__all(p))
#define DS_UNIFORM(x) (__builtin_amdgcn_readfirstlane(x))
#else
#define DS_WAVE_ANY(p) (p)
#define DS_WAVE_ALL(p) (p)
#define DS_UNIFORM(x) (x)
#endif

S2K_HD int ds_ctz32(u32 x) { return __builtin_ctz(x | 0x80000000u); }         // <= 31 also for x = 0

// 30 division steps on the low words.  zeta = -(delta + 1/2).  Returns the new zeta and the transition matrix
// t = (u v; q r) scaled by 2^30:  2^30 * (f', g') = t * (f, g).
S2K_HD int32_t ds_batch(int32_t zeta, u32 f, u32 g, int32_t t[4]) {
    int32_t u = 1, v = 0, q = 0, r = 1;
    int left = DS_BITS;
    while (DS_WAVE_ANY(left > 0)) {
        // the whole run of even g in one go: g/2^z, delta + z, f's row of the matrix catches up by 2^z
        int z = ds_ctz32(g); z = z < left ? z : left;
        g >>= z; u = (int32_t)((u32)u << z); v = (int32_t)((u32)v << z); zeta -= z; left -= z;
        // one step with g odd (lanes with steps left): delta > 0 swaps, (f, g) <- (g, (g - f)/2), else g <- (g + f)/2
        const int act = left > 0;
        const int sw = act & (zeta < 0);
        const u32 fm = sw ? 0u - f : f;
        const int32_t um = sw ? -u : u, vm = sw ? -v : v;
        const u32 g2 = (g + fm) >> 1;
        const int32_t q2 = q + um, r2 = r + vm;
        f = sw ? g : f; u = sw ? q : u; v = sw ? r : v;
        g = act ? g2 : g; q = act ? q2 : q; r = act ? r2 : r;
        zeta = sw ? -zeta - 2 : zeta - act;
        u = (int32_t)((u32)u << act); v = (int32_t)((u32)v << act); left -= act;
    }
    t[0] = u; t[1] = v; t[2] = q; t[3] = r;
    return zeta;
}

// The same 30 steps when zeta, f and g are the same in every lane (ds_inverse_words<true>): the values live in scalar registers, so
// the loop is scalar code that branches on its data where ds_batch has to select (no vote, no divergence; ~15 instructions a trip
// instead of ~50 in the select form).
S2K_HD int32_t ds_batch_uniform(int32_t zeta, u32 f, u32 g, int32_t t[4]) {
    int32_t u = 1, v = 0, q = 0, r = 1;
    int left = DS_BITS;
    for (;;) {
        int z = ds_ctz32(g); z = z < left ? z : left;
        g >>= z; u = (int32_t)((u32)u << z); v = (int32_t)((u32)v << z); zeta -= z; left -= z;
        if (left <= 0) break;
        if (zeta < 0) {                                     // swap: (f, g, u, v, q, r) <- (g, (g - f)/2, q, r, q - u, r - v)
            const u32 f0 = f; const int32_t u0 = u, v0 = v;
            f = g; u = q; v = r;
            g = (g - f0) >> 1; q -= u0; r -= v0;
            zeta = -zeta - 2;
        } else {
            g = (g + f) >> 1; q += u; r += v;
            zeta -= 1;
        }
        u = (int32_t)((u32)u << 1); v = (int32_t)((u32)v << 1); left -= 1;
    }
    t[0] = u; t[1] = v; t[2] = q; t[3] = r;
    return zeta;
}

// (a, b) <- (t00 a + t01 b + ka m, t10 a + t11 b + kb m) / 2^30.  WITH_M = false: the exact (f, g) update (ka = kb = 0, the
// low 30 bits vanish by construction); WITH_M = true: the (d, e) update, ka / kb in [0, 2^30) clear the low 30 bits.
template <bool WITH_M>
S2K_HD void ds_apply(ds_int& a, ds_int& b, const int32_t t[4], const ds_modulus md) {
    const int64_t t00 = t[0], t01 = t[1], t10 = t[2], t11 = t[3];
    int64_t ca = t00 * a.w[0] + t01 * b.w[0], cb = t10 * a.w[0] + t11 * b.w[0];
    int64_t ka = 0, kb = 0;
    if (WITH_M) {
        ka = (int64_t)((0u - (u32)ca * md.inv) & (u32)DS_MASK);            // ka * m == -ca  (mod 2^30)
        kb = (int64_t)((0u - (u32)cb * md.inv) & (u32)DS_MASK);
        ca += ka * md.w[0]; cb += kb * md.w[0];
    }
    ca >>= DS_BITS; cb >>= DS_BITS;
#pragma unroll
    for (int i = 1; i < DS_LIMBS; i++) {
        ca += t00 * a.w[i] + t01 * b.w[i];
        cb += t10 * a.w[i] + t11 * b.w[i];
        if (WITH_M && md.w[i] != 0) { ca += ka * md.w[i]; cb += kb * md.w[i]; }
        a.w[i - 1] = (int32_t)ca & DS_MASK; ca >>= DS_BITS;
        b.w[i - 1] = (int32_t)cb & DS_MASK; cb >>= DS_BITS;
    }
    a.w[DS_LIMBS - 1] = (int32_t)ca; b.w[DS_LIMBS - 1] = (int32_t)cb;
}

// r <- r + c * m, carries propagated (|c| small)
S2K_HD void ds_add_multiple(ds_int& r, int32_t c, const ds_modulus md) {
    int64_t acc = 0;
#pragma unroll
    for (int i = 0; i < DS_LIMBS - 1; i++) { acc += (int64_t)r.w[i] + (int64_t)c * md.w[i]; r.w[i] = (int32_t)acc & DS_MASK; acc >>= DS_BITS; }
    r.w[DS_LIMBS - 1] = (int32_t)(acc + r.w[DS_LIMBS - 1] + (int64_t)c * md.w[DS_LIMBS - 1]);
}

// The end of an inversion: g = 0, f = +-gcd = +-1 (or f = +-m when the input was 0, with d = 0), and d * input == f (mod m), |d| < 21 m.
// f's top limb carries f's sign; d may come in any limb form ds_add_multiple takes.  o <- the inverse in [0, m) as 8 words.
S2K_HD void ds_finish_words(u32 o[8], const ds_int& f, ds_int& d, const ds_modulus md) {
    // r = d + 32 m > 0; quotient estimate q = r >> 256 (m = 2^256 - c, c < 2^129, so r - q m = (r mod 2^256) + q c < 2 m)
    ds_add_multiple(d, 32, md);
    const int32_t qest = d.w[DS_LIMBS - 1] >> 16;
    ds_add_multiple(d, -qest, md);
    { ds_int s = d; ds_add_multiple(s, -1, md); const int keep = s.w[DS_LIMBS - 1] >= 0;                 // one conditional subtraction
#pragma unroll
      for (int i = 0; i < DS_LIMBS; i++) d.w[i] = keep ? s.w[i] : d.w[i]; }
    // sign of f: a negative f means the inverse is -d = m - d (for d != 0)
    { const int fneg = f.w[DS_LIMBS - 1] < 0;
      int32_t nz = 0;
#pragma unroll
      for (int i = 0; i < DS_LIMBS; i++) nz |= d.w[i];
      ds_int s;
#pragma unroll
      for (int i = 0; i < DS_LIMBS; i++) s.w[i] = -d.w[i];
      // -d + m, limbs renormalised
      int64_t acc = 0;
#pragma unroll
      for (int i = 0; i < DS_LIMBS - 1; i++) { acc += (int64_t)s.w[i] + md.w[i]; s.w[i] = (int32_t)acc & DS_MASK; acc >>= DS_BITS; }
      s.w[DS_LIMBS - 1] = (int32_t)(acc + s.w[DS_LIMBS - 1] + md.w[DS_LIMBS - 1]);
      const int take = fneg & (nz != 0);
#pragma unroll
      for (int i = 0; i < DS_LIMBS; i++) d.w[i] = take ? s.w[i] : d.w[i]; }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int bit = 32 * j, i = bit / DS_BITS, sh = bit % DS_BITS;
        u64 v = (u64)(u32)d.w[i] >> sh;
        if (i + 1 < DS_LIMBS) v |= (u64)(u32)d.w[i + 1] << (DS_BITS - sh);
        if (i + 2 < DS_LIMBS) v |= (u64)(u32)d.w[i + 2] << (2 * DS_BITS - sh);
        o[j] = (u32)v;
    }
}

// w (8 little-endian 32-bit words, value < m) -> w^-1 mod m (0 for 0).
// UNIFORM = true: w is the same in every lane of the wavefront (waveinv.h).  The batch kernel then takes the low words of f and g
// through v_readfirstlane and runs on the scalar unit (ds_batch_uniform); so, as the compiler sees that everything else is uniform
// too, does ds_apply (s_mul_i32 / s_mul_hi_i32 pairs).
template <bool UNIFORM = false>
S2K_HD void ds_inverse_words(u32 o[8], const u32 w[8], const ds_modulus md) {
    ds_int f, g, d, e;
#pragma unroll
    for (int i = 0; i < DS_LIMBS; i++) {
        const int bit = DS_BITS * i, idx = bit >> 5, sh = bit & 31;
        u64 v = w[idx];
        if (idx + 1 < 8) v |= (u64)w[idx + 1] << 32;
        g.w[i] = (int32_t)((u32)(v >> sh) & (u32)DS_MASK);
        f.w[i] = md.w[i]; d.w[i] = 0; e.w[i] = 0;
    }
    e.w[0] = 1;
    int32_t zeta = -1;
#pragma unroll 1
    for (int it = 0; it < DS_BATCHES; it++) {
        int32_t t[4];
        if (UNIFORM) zeta = ds_batch_uniform(DS_UNIFORM(zeta), (u32)DS_UNIFORM(f.w[0]), (u32)DS_UNIFORM(g.w[0]), t);
        else zeta = ds_batch(zeta, (u32)f.w[0], (u32)g.w[0], t);
        ds_apply<true>(d, e, t, md);
        ds_apply<false>(f, g, t, md);
        // 590 steps is the worst case; random inputs are through after 501..531 of them (18 batches).  Once g = 0 a further batch leaves f
        // and d as they are (its matrix is diag(2^30, 1): d <- (2^30 d + 0 m) / 2^30), so stopping when EVERY lane of the wavefront has
        // g = 0 gives bit for bit the result of running all 20 batches.
        if (it >= DS_BATCHES - 5) {
            int32_t gz = 0;
#pragma unroll
            for (int i = 0; i < DS_LIMBS; i++) gz |= g.w[i];
            if (DS_WAVE_ALL(gz == 0)) break;
        }
    }
    ds_finish_words(o, f, d, md);
}

#if defined(__HIPCC__)
// ---- the uniform inverse with its state across the lanes (device only) ----------------------------------------------------------------
// ds_inverse_words<true> keeps f, g, d, e in scalar registers and walks their limbs one after the other: ~650 dependent scalar
// instructions per batch for the two matrix applications.  Here lane i (0..8) of the wavefront holds limb i of each of the four
// numbers, lanes 9..63 hold zeros and ride along, and a matrix application is three (d, e) or two (f, g) v_mad_i64_i32 per number in
// all lanes at once.  The batch kernel stays on the scalar unit (ds_batch_uniform on lane 0's f and g, v_readlane); so does the
// choice of ka, kb, from lane 0's d and e, as in ds_apply<true>.
//
// Carries.  Lane i forms S_i = t00 a_i + t01 b_i (+ ka m_i); the new number is (sum S_i 2^(30 i)) / 2^30, and S_0 = 0 mod 2^30.  S_i is
// cut into lo = S_i mod 2^30, mid = (S_i >> 30) mod 2^30 and top = S_i >> 60, and
//      u_j  = lo(S_(j+1)) + mid(S_j)                      in [0, 2^31 - 2]              (lo comes down one lane: the division by 2^30)
//      a'_j = (u_j mod 2^30) + (u_(j-1) >> 30) + top(S_(j-1))                            (the carry goes up one lane)
// Lane 8 keeps its whole signed S_8 >> 30 (no mask, no carry out), so lanes 9.. stay 0.  That is one and a half carry passes and two DPP
// moves per number.  Bound: |t00| + |t01| <= 2^30 for a matrix of 30 division steps, |m_i| < 2^30, 0 <= ka < 2^30, so with limbs
// |a_i| <= 2^30 + 3 going in, |S_i| <= 2^30 (2^30 + 3) + 2^30 (2^30 - 1) = 2^61 + 2^31: top is in [-3, 2], the carry in [-3, 3], and
//      limbs 0..7 come out in [-3, 2^30 + 2], limb 0 in [0, 2^30) exactly (nothing is carried into it),
// which is the bound going in again (the moduli's own limbs, the state of f before the first batch, are below 2^30 in size).  The
// limbs between batches are therefore redundant: a number is the sum of its limbs, not their concatenation, and the sign of the top
// limb is the number's only after the carry pass that the final reduction starts with.  The VALUES of f, g, d, e after every batch
// are those of ds_inverse_words<true> (ka depends only on d, e mod 2^30), so |d|, |e| < 21 m as in the header of this file, the top
// limb stays below 2^22 in size, and the result is bit for bit the same.  tests/test_cpu_wave_inverse_lanes.py runs a model of this
// scheme with explicit 64-bit wraparound and asserts the ranges; that test guards the bound.
//
// All 64 lanes must be active and call it in lock step with the same w.  The lane index is threadIdx.x & 63 (as wi_lane, waveinv.h):
// one-dimensional workgroups.
S2K_D int32_t dsl_from_below(int32_t x) { return __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true); }     // row_shr:1: lane i <- lane i - 1, 0 into lane 0
S2K_D int32_t dsl_from_above(int32_t x) { return __builtin_amdgcn_update_dpp(0, x, 0x101, 0xf, 0xf, true); }     // row_shl:1: lane i <- lane i + 1
// column sums -> limbs.  lm: 2^30 - 1 in lanes 0..7, all ones above; cm: all ones in lanes 0..7, 0 above.
S2K_D int32_t dsl_carry(int64_t s, int32_t lm, int32_t cm) {
    const int32_t lo = (int32_t)s & DS_MASK, mid = (int32_t)(s >> DS_BITS) & lm, top = (int32_t)(s >> (2 * DS_BITS));
    const int32_t u = dsl_from_above(lo) + mid;
    const int32_t c = ((u >> DS_BITS) + top) & cm;
    return (u & lm) + dsl_from_below(c);
}
S2K_D void dsl_gather(ds_int& r, int32_t v) {
#pragma unroll
    for (int i = 0; i < DS_LIMBS; i++) r.w[i] = __builtin_amdgcn_readlane(v, i);
}

// dump (DUMP only): after batch `it`, lanes 0..8 write limb `lane` of f, g, d, e to dump[(4 it + {0, 1, 2, 3}) 9 + lane]; *batches gets
// the number of batches run.  For tests/wave_inverse.
template <bool DUMP = false>
S2K_D void ds_inverse_words_lanes(u32 o[8], const u32 w[8], const ds_modulus md, int32_t* dump = nullptr, int* batches = nullptr) {
    const u32 lane = (u32)(threadIdx.x & 63u);
    const int32_t lm = lane < DS_LIMBS - 1 ? DS_MASK : -1, cm = lane < DS_LIMBS - 1 ? -1 : 0;
    int32_t m = 0, f, g = 0, d = 0, e = lane == 0 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < DS_LIMBS; i++) {
        const int bit = DS_BITS * i, idx = bit >> 5, sh = bit & 31;
        u64 v = w[idx];
        if (idx + 1 < 8) v |= (u64)w[idx + 1] << 32;
        g = lane == (u32)i ? (int32_t)((u32)(v >> sh) & (u32)DS_MASK) : g;
        if (md.w[i] != 0) m = lane == (u32)i ? md.w[i] : m;
    }
    f = m;
    int32_t zeta = -1;
    int it = 0;
#pragma unroll 1
    for (; it < DS_BATCHES; it++) {
        int32_t t[4];
        zeta = ds_batch_uniform(DS_UNIFORM(zeta), (u32)__builtin_amdgcn_readlane(f, 0), (u32)__builtin_amdgcn_readlane(g, 0), t);
        const u32 d0 = (u32)__builtin_amdgcn_readlane(d, 0), e0 = (u32)__builtin_amdgcn_readlane(e, 0);
        const int32_t ka = (int32_t)((0u - ((u32)t[0] * d0 + (u32)t[1] * e0) * md.inv) & (u32)DS_MASK);      // ka * m == -(t00 d + t01 e)  (mod 2^30)
        const int32_t kb = (int32_t)((0u - ((u32)t[2] * d0 + (u32)t[3] * e0) * md.inv) & (u32)DS_MASK);
        const int64_t sd = (int64_t)t[0] * d + (int64_t)t[1] * e + (int64_t)ka * m, se = (int64_t)t[2] * d + (int64_t)t[3] * e + (int64_t)kb * m;
        const int64_t sf = (int64_t)t[0] * f + (int64_t)t[1] * g, sg = (int64_t)t[2] * f + (int64_t)t[3] * g;
        d = dsl_carry(sd, lm, cm); e = dsl_carry(se, lm, cm);
        f = dsl_carry(sf, lm, cm); g = dsl_carry(sg, lm, cm);
        if (DUMP) {
            if (lane < DS_LIMBS) {
                int32_t* p = dump + (size_t)4 * DS_LIMBS * it + lane;
                p[0] = f; p[DS_LIMBS] = g; p[2 * DS_LIMBS] = d; p[3 * DS_LIMBS] = e;
            }
        }
        // as in ds_inverse_words: once g = 0 further batches change nothing.  A g that is 0 mostly arrives in redundant form (a limb of
        // 2^30 under limbs of 2^30 - 1 and one of -1, moving up a lane per batch), so the test is made on a copy with its carries
        // rippled all the way: 8 steps of one lane each bring limbs 0..7 to [0, 2^30), and then every limb 0 is g = 0.
        if (it >= DS_BATCHES - 5) {
            int32_t z = g;
#pragma unroll
            for (int k = 0; k < DS_LIMBS - 1; k++) z = (z & lm) + dsl_from_below((z >> DS_BITS) & cm);
            if (__all(z == 0)) { it++; break; }
        }
    }
    if (DUMP) *batches = it;
    // the limbs back into every lane (uniform: the rest is scalar code, once per inversion), f brought to canonical limbs for its sign
    ds_int fw, dw;
    dsl_gather(fw, f); dsl_gather(dw, d);
    ds_add_multiple(fw, 0, md);
    ds_finish_words(o, fw, dw, md);
}
#endif
