// tests/gpu_prims/ring_step_trim_forms.h -- TEST INFRASTRUCTURE ONLY.
// The three signed-accumulator forms of group.h on coordinates given as raw limbs, the same few lines for the host emulation
// (tests/host_emul/ring_step_trim_emu.cpp) and the device (ring_step_trim_prims.hip), so that the two can be compared limb for limb.
#pragma once

S2K_HD void trim_load(fe& r, const u32* w) {
    for (int i = 0; i < 9; i++) r.n[i] = w[i];
}
S2K_HD void trim_store(u32* w, const fe& a) {
    for (int i = 0; i < 9; i++) w[i] = a.n[i];
}
S2K_HD void trim_dbl(gej& r, const gej& a, int nx) {
    if (nx) gej_dblneg_ring<true>(r, a); else gej_dblneg_ring<false>(r, a);
}
S2K_HD int trim_rsub(gej& r, const gej& a, const ge& b) { return gej_rsub_ge_ring(r, a, b); }
S2K_HD void trim_gez(gez& a, const ge& b) { gez_add_ge_ring(a, b); }
