// waveinv.h -- the field inverses of all 64 lanes of a wavefront for the price of one: Montgomery's trick across the lanes, and the
// one inversion that is left run with its division-step control on the scalar unit.
//
// Every lane of a to-affine step (rp_rings_shared) runs fe_inv on its own Z, so a wavefront pays for 64 inversions in the instruction
// stream of one: ~19 000 VALU wave-instructions per ring position.  Here instead:
//   * prefix and suffix products over the 64 lanes (Hillis-Steele, 6 steps each, both scans in one lock-step product pair per step;
//     the 9 limbs of a neighbour come through ds_bpermute, which takes no VALU slot): lane l holds z_0 .. z_l and z_l .. z_63;
//   * P = z_0 .. z_63 is inverted ONCE.  Its value is the same in every lane, so the 30-step batch kernel of modinv.h, which only looks
//     at the low words of f and g, takes them through v_readfirstlane and compiles to s_* arithmetic with no wave vote
//     (ds_batch_uniform): it runs on the scalar unit, idle in this kernel, while the sibling wave keeps the VALU.  The four numbers of
//     the inversion lie across the lanes, one limb each, and the matrix application is a few v_mad_i64_i32 and DPP moves per batch
//     (ds_inverse_words_lanes, modinv.h; -DS2K_WAVEINV_SCALAR_APPLY selects the earlier form, ds_apply on the scalar unit too:
//     ~19 000 dependent scalar instructions per inversion);
//   * 1/z_l = P^-1 . (z_0 .. z_(l-1)) . (z_(l+1) .. z_63).
// Values are exactly those of fe_inv (the inverse is unique).  If any lane's z is 0 mod p, P is 0 and every lane gets 0 back as the
// return value (the outputs are then meaningless).  Magnitude contract: z <= 2, as fe_inv; outputs have magnitude 1.
// All 64 lanes must be active and call it in lock step.
// Device only: the host build (tests/host_emul) inverts per lane (fe_inv_lanes).
#pragma once
#include "fe.h"

#if defined(__HIPCC__)                      /* both passes of hipcc see the declarations; the wave routines are __device__ */
S2K_D u32 wi_lane() { return (u32)(threadIdx.x & 63u); }
S2K_D void wi_fetch(fe& r, const fe& a, u32 src) {              // r = lane src's a (src in 0..63)
    const int addr = (int)(src << 2);
#pragma unroll
    for (int i = 0; i < FE_LIMBS; i++) r.n[i] = (u32)__builtin_amdgcn_ds_bpermute(addr, (int)a.n[i]);
}
#if defined(S2K_WAVEINV_SCALAR_APPLY)          /* the form before the lane-distributed one as the default: A/B libraries */
#define WI_SCALAR_APPLY true
#else
#define WI_SCALAR_APPLY false
#endif
template <bool SCALAR_APPLY = WI_SCALAR_APPLY>
S2K_D int fe_inv_wave(fe& r, const fe& z) {
    const u32 l = wi_lane();
    fe pre = z, suf = z;
#pragma unroll
    for (int s = 0; s < 6; s++) {
        const u32 d = 1u << s;
        fe a, b, pa, sb;
        wi_fetch(a, pre, (l - d) & 63u);
        wi_fetch(b, suf, (l + d) & 63u);
        fe_mul2(pa, pre, a, sb, suf, b);                        // magnitudes (<= 2) x (<= 2)
        fe_cmov(pre, pa, l >= d);
        fe_cmov(suf, sb, l + d < 64u);
    }
    fe e, s, one, q, P;
    fe_set_int(one, 1);
    wi_fetch(e, pre, (l - 1u) & 63u); fe_cmov(e, one, l == 0u);     // z_0 .. z_(l-1)
    wi_fetch(s, suf, (l + 1u) & 63u); fe_cmov(s, one, l == 63u);    // z_(l+1) .. z_63
    fe_mul(q, e, s);
    wi_fetch(P, pre, 63u);                                      // the same in every lane
    fe_normalize(P);
    const int ok = !fe_is_zero_normalized(P);
    u32 w[8], o[8]; fe_to_words(w, P);
    if (SCALAR_APPLY) ds_inverse_words<true>(o, w, DS_MOD_P);
    else ds_inverse_words_lanes(o, w, DS_MOD_P);
    fe ip; fe_from_words(ip, o);
    fe_mul(r, ip, q);
    return ok;
}
#endif

// r = 1/z for every lane of a wavefront (all 64 lanes, in lock step).  Returns 0 when some lane's z is 0 mod p (on the host: this
// lane's).  Device: fe_inv_wave; host build: fe_inv per lane.
S2K_HD int fe_inv_lanes(fe& r, const fe& z) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_inv_wave(r, z);
#else
    fe_inv(r, z);
    return !fe_normalizes_to_zero(z);
#endif
}
