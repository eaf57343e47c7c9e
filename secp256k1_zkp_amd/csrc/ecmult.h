// ecmult.h -- per-lane double multiplication  R = na*A + ng*G  (the reference's secp256k1_ecmult,
// src/ecmult_impl.h:365-375 -> strauss_wnaf :252-363) re-designed for a 64-wide SIMT machine.
//
// The reference interleaves wNAF(5) of the GLV halves of na with wNAF(15) of ng and walks 129 doublings; its per-call
// table (8 odd multiples + lambda copies) lives on the CPU stack.  On gfx950 a sparse wNAF wastes lanes -- an add slot
// costs the whole wavefront whenever ANY lane has a digit -- so every slot is made useful for every lane:
//
//   variable point:  GLV split (scalar.h); each 129-bit half is recoded into 33 signed ODD 4-bit digits (never zero;
//                    digit i is read straight off the bits of the scalar, no carry chain), so the loop is exactly
//                    4 doublings + 2 additions per digit position for all 64 lanes.  The 8 odd multiples {1..15}P
//                    (+ their beta*x for lambda*P) are built once per multiplication with one common Z -- the reference's
//                    isomorphic-curve / global-Z trick (ecmult_impl.h:73-115, group_impl.h:289-320) -- and parked in a
//                    per-lane 1152-byte slice of HBM (L2/MALL resident while the lane is alive); operands are gathered one
//                    addition ahead so the ~1-2 us of latency hides under the previous ~4 us of arithmetic.
//   generator:       no doublings at all: ng is cut into 10 signed digits of 26 bits (S2K_GTAB_BITS), each indexing a precomputed
//                    (window, |digit|) -> affine multiple table (gtable.h, 21.5 GB of the 288 GB of HBM), 10 mixed additions.
//   digits:          both digit streams live in LDS (lane_mem), not in registers.
//   control:         one loop whose body contains exactly ONE doubling site and ONE mixed-add site, driven by a
//                    per-lane micro-program counter.  The only data-dependent *arithmetic* case (P + P inside an add)
//                    becomes "take the operand and double it on the next trip", so exceptional inputs cost one extra
//                    trip for that lane instead of a second copy of the doubling code.
//
// Results are identical to the reference as group elements (and therefore as serialised bytes).
#pragma once
#include "group.h"
#include "scalar.h"

// ---- generator table ---------------------------------------------------------------------------------
// Fixed-base table of G (and, same layout, of a rangeproof generator): SIGNED digits of D = S2K_GTAB_BITS bits.  A scalar s < 2^256 is
// cut as  s = sum_w d_w 2^(D w)  with d_w in [-2^(D-1), 2^(D-1)) for every window but the top one (which takes what is left, >= 0):
// adding the constant K = sum_{w < W-1} 2^(D-1 + D w) once turns that into plain unsigned windows t_w of s' = s + K with d_w = t_w - 2^(D-1)
// (gtab_recode; s' has up to 257 bits: 9 words), so a window is still read straight off the stored words, with no carry chain.  The
// table holds v * 2^(D w) * G for v = 1 .. 2^(D-1) only -- a negative digit negates y when the operand is decoded -- i.e. HALF the entries
// an unsigned window of the same width needs: D = 26 gives W = 10 windows (one addition less per multiplication than the 11 unsigned
// 24-bit windows of rounds 1-3) in 10 x 2^25 x 64 B = 21.5 GB of the 288 GB; D = 24 would be 11 windows in 5.9 GB.
// Slot (w, v) = (w << (D-1)) + v: v = 2^(D-1) lands on slot (w+1, 0), which no window ever reads (a zero digit adds nothing).
// One entry = one aligned 64-byte sector of canonical words (x[8], y[8], least significant first), the same record format as the
// per-lane tables below, so that the main loops have a single operand pipeline.  (The host emulation builds D = 12.)
// Round 5: the width D is a property of the TABLE, not of the code -- the engine builds D = 26 where 21.5 GB are to be had and falls back to
// narrower tables where they are not (24: 5.9 GB, 22: 1.6 GB, 20: 0.44 GB; one more addition per multiplication for every step down; the
// reference's knob of the same kind is ECMULT_WINDOW_SIZE, src/ecmult.h:14-38).  Slot (0, 0) -- the only slot no digit ever addresses and
// no entry is stored in -- is the table's header: word 0 = D, word 1 = the number of windows, words 2..10 = the recoding constant K.
// Every routine below takes its geometry from there (one uniform load per multiplication); S2K_GTAB_BITS is only the DEFAULT width.
#ifndef S2K_GTAB_BITS
#define S2K_GTAB_BITS 26
#endif
#define S2K_GTAB_MAX_BITS 26
#define S2K_GTAB_ENTRY_WORDS 16
#define S2K_GTAB_SWORDS 9           /* words of a recoded scalar */
#define S2K_GTAB_MAX_WINDOWS 32     /* D >= 8 */
struct gtab_geom { u32 D, W; };     // digit width, number of windows
S2K_HD u32 gtab_windows_for(u32 D) { return (256u + D - 1u) / D; }
S2K_HD u32 gtab_top_bits_for(u32 D) { return 256u - D * (gtab_windows_for(D) - 1u); }      // the top window's value is at most 2^TOP_BITS (its bits + the carry)
S2K_HD int gtab_bits_ok(u32 D) { return D >= 8u && D <= S2K_GTAB_MAX_BITS && gtab_top_bits_for(D) >= 1u && gtab_top_bits_for(D) < D - 1u; }      // the top window must fit the table
S2K_HD size_t gtab_slot(u32 D, u32 w, u32 v) { return ((size_t)w << (D - 1u)) + (size_t)v; }
S2K_HD size_t gtab_slots_for(u32 D) { return gtab_slot(D, gtab_windows_for(D), 0) + 1; }
S2K_HD size_t gtab_words_for(u32 D) { return gtab_slots_for(D) * S2K_GTAB_ENTRY_WORDS; }
S2K_HD gtab_geom gtab_geometry(const u32* tab) { gtab_geom g; g.D = tab[0]; g.W = tab[1]; return g; }
// the header of a table of width D (written once, by the kernel that builds the window bases)
S2K_HD void gtab_write_header(u32* tab, u32 D) {
    const u32 W = gtab_windows_for(D);
    tab[0] = D; tab[1] = W;
    for (int i = 0; i < S2K_GTAB_SWORDS; i++) {
        u32 k = 0;
        for (u32 w = 0; w + 1 < W; w++) { const u32 bit = D - 1u + D * w; if ((bit >> 5) == (u32)i) k |= 1u << (bit & 31u); }
        tab[2 + i] = k;
    }
    for (int i = 2 + S2K_GTAB_SWORDS; i < S2K_GTAB_ENTRY_WORDS; i++) tab[i] = 0;
}

S2K_HD void gtab_load(ge& r, const u32* gtab, u32 window, u32 v) {
    const u32* p = gtab + gtab_slot(gtab[0], window, v) * S2K_GTAB_ENTRY_WORDS;
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = p[i];
    fe_from_words(r.x, w); fe_from_words(r.y, w + 8);
}
// s (8 little-endian words) -> s' = s + K (9 words), K from the header of the table the digits will index
S2K_HD void gtab_recode(u32 out[S2K_GTAB_SWORDS], const u32 s[8], const u32* tab) {
    u64 cy = 0;
#pragma unroll
    for (int i = 0; i < S2K_GTAB_SWORDS; i++) {
        cy += (u64)(i < 8 ? s[i] : 0u) + tab[2 + i];
        out[i] = (u32)cy; cy >>= 32;
    }
}
// window g of a recoded scalar, given the two words that hold its bits (lo = word (D g) >> 5, hi = the next one or 0): the table record to
// add (returns 0: the digit is zero) and whether its y has to be negated
S2K_HD int gtab_locate(const u32*& addr, int& neg, const u32* tab, const gtab_geom& G, int g, u32 lo, u32 hi) {
    const u32 b = (u32)g * G.D;
    const u64 pair = (u64)lo | ((u64)hi << 32);
    const u32 t = (u32)(pair >> (b & 31u)) & ((1u << G.D) - 1u);
    u32 v;
    if ((u32)g + 1u < G.W) { const int d = (int)t - (int)(1u << (G.D - 1u)); neg = d < 0; v = (u32)(d < 0 ? -d : d); }
    else { neg = 0; v = t; }
    if (!v) return 0;
    addr = tab + gtab_slot(G.D, (u32)g, v) * S2K_GTAB_ENTRY_WORDS;
    return 1;
}

// ---- per-lane table of odd multiples ----------------------------------------------------------------------
// ptab (this lane's slice of HBM, 128-byte aligned): entry e = 0..7 holds (2e+1)*P on the isomorphic curve as two
// 64-byte sectors of canonical 8x32-bit words,  [ x | y ]  and  [ beta*x | y ] , so that an operand for either GLV half
// is exactly ONE aligned 64-byte gather (the per-lane tables of all resident waves live in the Infinity Cache, not L2:
// every gather crosses the fabric, so sectors are what is paid for).  During construction the same 128 bytes hold the
// 27 limbs (x, y, z-ratio) of the not-yet-rescaled entry.
// S2K_PTAB_TWINS = 0 (default): only [ x | y ] is kept and an operand for the lambda half costs one multiplication by beta when it
// is decoded.  The finished tables of a lane are then 16 sectors = 1 KB (two-piece form) instead of 2 KB, i.e. 134 MB instead of
// 268 MB for the 131 072 resident lanes of a rangeproof launch -- inside the 256 MB Infinity Cache instead of just beyond it -- and
// the rescaling pass saves one product, one normalisation and half of its stores per entry.  S2K_PTAB_TWINS = 1 keeps [ beta*x | y ].
#ifndef S2K_PTAB_TWINS
#define S2K_PTAB_TWINS 0
#endif
#define S2K_PTAB_ENTRIES 8
#define S2K_PTAB_ENTRY_WORDS 32
#define S2K_PTAB_TABLE_WORDS (S2K_PTAB_ENTRIES * S2K_PTAB_ENTRY_WORDS)
#define S2K_PTAB_ZISO (2 * S2K_PTAB_TABLE_WORDS)          // parked while the main loop runs, to keep VGPRs for arithmetic
#define S2K_PTAB_NG (S2K_PTAB_ZISO + 9)
#define S2K_PTAB_WORDS (2 * S2K_PTAB_TABLE_WORDS + 32)    // two tables (the second one only in the split form below) + parked factors

// A parked entry is 27 words (x, y, third); WS = distance between its consecutive words: 1 for an entry that lies in one piece in the
// lane's own slice, 64 for the wave-interleaved parking area of the ring form (word k of the 64 lanes of a wavefront side by side, so
// that one store / load instruction moves 256 contiguous bytes instead of touching 64 different lines).
// Non-temporal hints for data that is touched once, so that it does not displace the finished per-lane tables (2 KB per lane, re-read ~50
// times per ring position, 268 MB over the resident lanes: right at the size of the Infinity Cache) from the caches.  S2K_NT_PARK: the parked
// entries of a table under construction in the ring form's SEPARATE, wave-interleaved parking area (written once, read once by the rescaling
// pass; NOT the in-place parking of the general form, whose lines the finished sectors overwrite at once: hinted, it lost 15 %); S2K_NT_GTAB: the operands the shared-generator
// ring form takes from the 21.5 GB fixed-base tables (random sectors, never reused).  Measured together on one box (tools/ab_probe.py,
// profiles/r04v_ab_nontemporal.txt): 1.0425e6 -> 1.053e6 verifies/s; either one alone is inside the noise (+-0.4 %).  0 = plain accesses.
#if defined(__HIP_DEVICE_COMPILE__)
#define S2K_LD_NT(p) __builtin_nontemporal_load(p)
#define S2K_ST_NT(v, p) __builtin_nontemporal_store((v), (p))
#else
#define S2K_LD_NT(p) (*(p))
#define S2K_ST_NT(v, p) (*(p) = (v))
#endif
#ifndef S2K_NT_PARK
#define S2K_NT_PARK 1
#endif
// S2K_XYZZ_TABLE_PART: the run of fixed-base additions at the end of a multiplication (W from G's table, W more from the generator's in the
// ring form) has no doubling in between, so its accumulator can stay in extended Jacobian form (X, Y, ZZ, ZZZ: group.h): an addition then
// costs 8M + 2S instead of 8M + 3S, and the same-x test of every addition becomes ONE zero test of ZZ behind the run (an exceptional
// addition zeroes ZZ for good; additions of zero digits are not committed, so they cannot).  In: ZZ = Z^2, ZZZ = Z ZZ; out: (X ZZ, Y ZZZ, ZZ).
// A/B on one box, three alternating rounds (profiles/r05x_ab_xyzz_table_part.txt): general form (every proof its own generator) +0.9 % in
// every round, shared-generator form +0.3 % (inside its noise), BIP-340 (ecmult_lane: its table part is not a loop of its own) unchanged.
#ifndef S2K_XYZZ_TABLE_PART
#define S2K_XYZZ_TABLE_PART 1
#endif
#ifndef S2K_NT_GTAB_SPLIT
#define S2K_NT_GTAB_SPLIT 0      /* the same hint on the generator part of ecmult_lane_split (general form of the rings kernel): A/B in profiles/r05*_ab_* */
#endif
#ifndef S2K_NT_GTAB
#define S2K_NT_GTAB 1
#endif
template <int WS = 1>
S2K_HD void ptab_store_raw(u32* e, const fe& x, const fe& y, const fe& third) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        if (S2K_NT_PARK && WS > 1) { S2K_ST_NT(x.n[i], &e[i * WS]); S2K_ST_NT(y.n[i], &e[(9 + i) * WS]); S2K_ST_NT(third.n[i], &e[(18 + i) * WS]); }
        else { e[i * WS] = x.n[i]; e[(9 + i) * WS] = y.n[i]; e[(18 + i) * WS] = third.n[i]; }
    }
}
// Table construction in two passes.  ptab_build_raw: the odd multiples by co-Z additions of 2A, each entry parked as (x, y, z-ratio of
// its step) limbs; returns the Z all of them will share once rescaled (the Z of the last entry).  ptab_rescale: brings every entry to the Z of the last one times `zs0`
// (secp256k1_ge_table_set_globalz, group_impl.h:289-320) and packs it as canonical words with its beta*x twin.  zs0 = 1 for a
// single table; with two tables each is rescaled by the OTHER one's Z so that all sixteen entries share one Z (ecmult_lane_split).
template <int N, int WS = 1, int ES = S2K_PTAB_ENTRY_WORDS>
S2K_HD void ptab_build_raw_n(fe& ziso, u32* tab, const gej& A) {
    // 2A by the usual doubling, whose intermediates also give A itself at the Z of 2A for free: Z(2A) = Y Z, so A rescaled by Y is
    // (X Y^2, Y^4) = (-T, S^2).  From then on every odd multiple is a CO-Z addition of 2A (both operands share Z: 5M + 2S instead of the
    // 8M + 3S of a mixed addition, and 2A comes out rescaled to the sum's Z for the next step); the step's Z ratio is just X(2A) - X(P).
    fe x = A.x, y = A.y; fe_norm_weak(x); fe_norm_weak(y);
    fe zc, s, t, l, nx, s2, qx, qy, w, px, py;
    fe_mul_sqr(zc, y, A.z, s, y);                          // Z(2A) = Y Z, S = Y^2
    fe_neg(nx, x, 1);
    fe_mul_sqr(t, nx, s, l, x);                            // T = -X S, X^2
    fe_mul_int(l, 3); fe_half(l); fe_norm_weak(l);         // L = 3/2 X^2
    fe_sqr2(qx, l, s2, s);                                 // L^2, S^2
    fe_add(qx, t); fe_add(qx, t); fe_norm_weak(qx);        // X(2A)                                  (1)
    fe_add2(w, qx, t);
    fe_mul(qy, l, w); fe_add(qy, s2); fe_neg(qy, qy, 2); fe_norm_weak(qy);     // Y(2A) = -(L (X3 + T) + S^2)      (1)
    fe_neg(px, t, 1); py = s2;                             // A at the Z of 2A                      (2, 1)
    { fe one; fe_set_int(one, 1); ptab_store_raw<WS>(tab, px, py, one); }
    for (int i = 1; i < N; i++) {
        fe dx, dy, c, d, w1, w2, e, a1, x3, y3, tmp;
        fe_neg(dx, px, 4); fe_add(dx, qx); fe_norm_weak(dx);              // X(2A) - X(P): also Z(sum) / Z(operands)
        fe_neg(dy, py, 3); fe_add(dy, qy); fe_norm_weak(dy);
        fe_sqr2(c, dx, d, dy);
        fe_mul2(w1, qx, c, w2, px, c);                                    // (1*1, 4*1)
        fe_neg(e, w2, 1); fe_add(e, w1);                                  // W1 - W2                     (3)
        fe_add2(tmp, w1, w2); fe_neg(tmp, tmp, 2);                        // -(W1 + W2)                  (3)
        fe_add2(x3, d, tmp);                                              // X(P + 2A)                   (4)
        fe_neg(tmp, x3, 4); fe_add(tmp, w1);                              // W1 - X3                     (6)
        fe_mul2(a1, qy, e, y3, dy, tmp);                                  // (1*3, 1*6)
        fe_neg(tmp, a1, 1); fe_add(y3, tmp);                              // Y(P + 2A)                   (3)
        fe_mul(zc, zc, dx);
        ptab_store_raw<WS>(tab + i * ES, x3, y3, dx);                      // third slot: z ratio of this step
        px = x3; py = y3; qx = w1; qy = a1;                               // 2A rescaled to the new Z
    }
    ziso = zc;
}
S2K_HD void ptab_build_raw(fe& ziso, u32* tab, const gej& A) { ptab_build_raw_n<S2K_PTAB_ENTRIES>(ziso, tab, A); }
// N parked entries at `tab` (one per S2K_PTAB_ENTRY_WORDS slot) -> N finished 64-byte sectors at fin + i * fin_stride.  fin == tab with
// fin_stride == S2K_PTAB_ENTRY_WORDS is the in-place form (a finished sector overwrites the head of its own parked entry, which has
// been taken over into registers by then).
template <int N, int WS = 1, int ES = S2K_PTAB_ENTRY_WORDS>
S2K_HD void ptab_rescale_n(u32* tab, u32* fin, int fin_stride, const fe* zs0) {
    fe zs; if (zs0) zs = *zs0; else fe_set_int(zs, 1);
    // The parked entry of step i-1 is requested before the arithmetic of step i and taken over after it (the first use of the loaded
    // words is where the wait lands; x, y, h are a second register set, so no copy of in-flight data sits at the loop head).  Exactly
    // 27 words are loaded: a 28th, dead, destination register would be recycled by the allocator while the load is in flight, and
    // the write-after-write hazard then puts a full wait right behind the request.
    u32 nraw[27];
    fe x, y, h;
#pragma unroll
    for (int k = 0; k < 27; k++) nraw[k] = (S2K_NT_PARK && WS > 1) ? S2K_LD_NT(&tab[(N - 1) * ES + k * WS]) : tab[(N - 1) * ES + k * WS];
#pragma unroll
    for (int k = 0; k < 9; k++) { x.n[k] = nraw[k]; y.n[k] = nraw[9 + k]; h.n[k] = nraw[18 + k]; }
    for (int i = N - 1; i >= 0; i--) {
        const u32* er = tab + i * ES;
        u32* e = fin + i * fin_stride;
        if (i > 0) {
#pragma unroll
            for (int k = 0; k < 27; k++) nraw[k] = (S2K_NT_PARK && WS > 1) ? S2K_LD_NT(&er[k * WS - ES]) : er[k * WS - ES];
        }
        if (zs0 || i != N - 1) {
            fe zs2, zs3; fe_sqr(zs2, zs); fe_mul(zs3, zs2, zs);
            fe_mul(x, x, zs2); fe_mul(y, y, zs3);
        }
        fe_normalize(x); fe_normalize(y);
        u32 wx[8], wy[8];
        fe_to_words(wx, x); fe_to_words(wy, y);
#pragma unroll
        for (int k = 0; k < 8; k++) { e[k] = wx[k]; e[8 + k] = wy[k]; }
#if S2K_PTAB_TWINS
        {
            fe beta, bx; fe_set_beta(beta);
            fe_mul(bx, x, beta); fe_normalize(bx);
            u32 wb[8]; fe_to_words(wb, bx);
#pragma unroll
            for (int k = 0; k < 8; k++) { e[16 + k] = wb[k]; e[24 + k] = wy[k]; }
        }
#endif
        fe_mul(zs, zs, h);             // ratio z_i / z_{i-1} joins the running product for the entries below
        if (i > 0) {
#pragma unroll
            for (int k = 0; k < 27; k++) S2K_CHAIN(nraw[k]);
#pragma unroll
            for (int k = 0; k < 9; k++) { x.n[k] = nraw[k]; y.n[k] = nraw[9 + k]; h.n[k] = nraw[18 + k]; }
        }
    }
}
S2K_HD void ptab_rescale(u32* tab, const fe* zs0) { ptab_rescale_n<S2K_PTAB_ENTRIES>(tab, tab, S2K_PTAB_ENTRY_WORDS, zs0); }
// Builds the table for a finite Jacobian A (magnitudes <= (5,3,1)); returns the factor that takes the accumulator's Z
// from the table's common-Z frame back to the real curve.  ~105 field multiplications.
S2K_HD void ptab_build(fe& ziso, u32* ptab, const gej& A) {
    ptab_build_raw(ziso, ptab, A);
    ptab_rescale(ptab, nullptr);
}
S2K_HD void ptab_load_ziso(fe& zi, const u32* ptab) {
#pragma unroll
    for (int i = 0; i < 9; i++) zi.n[i] = ptab[S2K_PTAB_ZISO + i];
}

// ---- wave-level predicates ------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define S2K_WAVE_ANY(p) (__any(p))
#define S2K_WAVE_ALL(p) (__all(p))
#define S2K_UNIFORM(x) (__builtin_amdgcn_readfirstlane(x))       /* a value known to be the same in every lane, as a scalar */
#else
#define S2K_WAVE_ANY(p) (p)
#define S2K_WAVE_ALL(p) (p)
#define S2K_UNIFORM(x) (x)
#endif

// Per-lane memory handed to ecmult_lane: the table slice in HBM and the digit stream in LDS.  The digit stream is what the
// main loop would otherwise carry in ~18 registers (two 160-bit digit shift registers and the 256-bit generator scalar) and
// spill around every point operation; in LDS it costs one ds_read per addition.  Word-major layout (word k of lane t at
// [k * S2K_DIG_STRIDE + t]) keeps the accesses bank-conflict free.
//   words 0..8 : 4-bit digit of addition a (2 <= a < 66) in nibble a & 7 of word a >> 3
//   words 9..17: ng recoded for the signed fixed-base windows (gtab_recode: 9 words); window g is bits [D g, D g + D)
#define S2K_DIG_WORDS 18
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) u32* s2k_lds_ptr;
#define S2K_DIG_STRIDE 256                  /* every kernel that calls ecmult_lane runs 256-lane workgroups */
#define S2K_LANE_DIG(shared_array) ((s2k_lds_ptr)(shared_array) + threadIdx.x)
#else
typedef u32* s2k_lds_ptr;
#define S2K_DIG_STRIDE 1
#define S2K_LANE_DIG(array) (array)
#endif
struct lane_mem { u32* ptab; s2k_lds_ptr dig; };

// 160-bit shift register holding a 129-bit magnitude: the next 4-bit digit window is always the top nibble
struct digit_reg { u32 w[5]; };
S2K_HD void digit_reg_init(digit_reg& r, const u32 k[5]) {          // k' << 31 : window of digit 31 (bits 125..128) at the top
    r.w[4] = (k[4] << 31) | (k[3] >> 1);
    r.w[3] = (k[3] << 31) | (k[2] >> 1);
    r.w[2] = (k[2] << 31) | (k[1] >> 1);
    r.w[1] = (k[1] << 31) | (k[0] >> 1);
    r.w[0] = (k[0] << 31);
}
S2K_HD u32 digit_reg_pop(digit_reg& r) {
    const u32 v = r.w[4] >> 28;
#pragma unroll
    for (int i = 4; i > 0; i--) r.w[i] = (r.w[i] << 4) | (r.w[i - 1] >> 28);
    r.w[0] <<= 4;
    return v;
}

#define S2K_ADDS_P 66            // 33 digit positions x 2 halves
#define S2K_ADD_G0 S2K_ADDS_P
#define S2K_ADDS_MAX (S2K_ADD_G0 + S2K_GTAB_MAX_WINDOWS)

// R = na*A + ng*G for this lane.  A is Jacobian (A.inf allowed), ng may be absent (has_ng = 0).
// gtab: generator table; ptab: this lane's private S2K_PTAB_WORDS-word slice of scratch memory.
// R is returned on the real curve, magnitudes (<=5,<=3,1).
S2K_HD void ecmult_lane(gej& R, const gej& A, const scalar& na, const scalar& ng, int has_ng, const u32* gtab, const lane_mem& lm) {
    u32* const ptab = lm.ptab; const s2k_lds_ptr dig = lm.dig;
    S2K_PROF_DECL;
    const int p_active = (!A.inf) & (!sc_is_zero(na));
    const int g_active = has_ng & (!sc_is_zero(ng));
    int hneg0, hneg1;
    fe ziso;
    {
        half_scalar h0, h1;
        sc_split_lambda_odd(h0, h1, na);                         // both magnitudes odd (< 2^129): no recoding correction
        hneg0 = h0.neg; hneg1 = h1.neg;
        {
            digit_reg dr0, dr1; digit_reg_init(dr0, h0.w); digit_reg_init(dr1, h1.w);
            u32 dw[9];
#pragma unroll
            for (int i = 0; i < 9; i++) dw[i] = 0;
#pragma unroll
            for (int i = 2; i < S2K_ADDS_P; i++) { const u32 v = (i & 1) ? digit_reg_pop(dr1) : digit_reg_pop(dr0); dw[i >> 3] |= v << ((i & 7) * 4); }
#pragma unroll
            for (int i = 0; i < 9; i++) dig[i * S2K_DIG_STRIDE] = dw[i];
        }
        S2K_PROF_MARK(1);
        if (S2K_WAVE_ANY(p_active)) {
            ptab_build(ziso, ptab, A);
#pragma unroll
            for (int i = 0; i < 9; i++) ptab[S2K_PTAB_ZISO + i] = ziso.n[i];
        }
    }
    const gtab_geom GG = gtab_geometry(gtab);
    {
        u32 ngr[S2K_GTAB_SWORDS]; gtab_recode(ngr, ng.d, gtab);
#pragma unroll
        for (int i = 0; i < S2K_GTAB_SWORDS; i++) dig[(9 + i) * S2K_DIG_STRIDE] = ngr[i];
    }

    S2K_PROF_MARK(2);
    // per-lane micro-program: additions a = 0..a_end-1, with 4 doublings in front of every even a in [2, 66)
    int a = p_active ? 0 : S2K_ADD_G0;
    int zfixed = !p_active;
    int dbl_left = 0, pending = 0;
    const int a_end = g_active ? S2K_ADD_G0 + (int)GG.W : S2K_ADD_G0;
    // Operand pipeline.  Every operand -- an odd multiple from this lane's table or a generator-table entry -- is one aligned
    // 64-byte record of canonical words (x, y).  `op_locate` turns an addition index into (record address, use it?, negate y?);
    // the record of addition a+1 is *requested* (16 words into `raw`, no use of the data) before the arithmetic of addition a
    // and *decoded* into limbs after it, so the gather's latency lies under ~1800 instructions instead of in front of them.
    // A lane that does not advance in a trip simply requests the same record again: no per-lane select ever waits on the data.
    auto op_locate = [&](const u32*& addr, int& valid, int& neg, int& lam, int idx) {
        addr = ptab; valid = 0; neg = 0; lam = 0;
        if (idx < S2K_ADD_G0) {
            const int h = idx & 1;
            const int hn = h ? hneg1 : hneg0;
            u32 v = 8u; int flip = hn; valid = 1;                                                   // top digit (a = 0, 1) is always +1
            if (idx >= 2 && idx < S2K_ADDS_P) v = (dig[(idx >> 3) * S2K_DIG_STRIDE] >> ((idx & 7) * 4)) & 15u;
            neg = (v < 8u) ^ flip;
            const u32 e = (v < 8u) ? (7u - v) : (v - 8u);
            addr = ptab + e * S2K_PTAB_ENTRY_WORDS + ((h && S2K_PTAB_TWINS) ? 16 : 0); lam = h && !S2K_PTAB_TWINS;
        } else if (idx < a_end) {
            const int g = idx - S2K_ADD_G0, w = (int)(((u32)g * GG.D) >> 5);
            valid = gtab_locate(addr, neg, gtab, GG, g, dig[(9 + w) * S2K_DIG_STRIDE], w + 1 < S2K_GTAB_SWORDS ? dig[(10 + w) * S2K_DIG_STRIDE] : 0u);
        }
    };
    auto op_decode = [&](ge& o, const u32 raw[16], int neg, int lam) {
        fe y, yn;
        fe_from_words(o.x, raw); fe_from_words(y, raw + 8);
        if (S2K_WAVE_ANY(lam)) {                                    // twin-less tables: the lambda half's x is beta * x
            fe beta, bx; fe_set_beta(beta); fe_mul(bx, o.x, beta);
            fe_select(o.x, bx, o.x, lam);
        }
        fe_neg(yn, y, 1);
        fe_select(o.y, yn, y, neg);
    };
    const u32* nxt_addr; int nxt_valid, nxt_neg, nxt_lam;
    u32 raw[16];
    ge cur; int cur_valid;
    op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, a);
#pragma unroll
    for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
    op_decode(cur, raw, nxt_neg, nxt_lam); cur_valid = nxt_valid;
    gej_set_infinity(R);
    if (p_active) {                                 // addition 0 would add the top digit of half 0 to infinity: just take it
        gej_set_ge(R, cur);
        a = 1;
        op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, a);
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
        op_decode(cur, raw, nxt_neg, nxt_lam); cur_valid = nxt_valid;
    }
    op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, a + 1);
    // Lock-step fast path.  When every lane of the wavefront multiplies a live point (and the lanes agree on whether there is a
    // generator part) they all sit at the same place of the same micro-program, so the schedule is a plain loop: no per-lane
    // program counter, no select after every point operation, lean formulas (group.h).  A lane that meets an operand with its
    // own x coordinate (P + P, P - P: adversarial inputs only) makes the wavefront leave the fast path *before* that addition
    // is committed; the general loop below picks up from exactly that state.
#ifndef S2K_NO_FAST_PATH
    if (S2K_WAVE_ALL(p_active) && (S2K_WAVE_ALL(g_active) || !S2K_WAVE_ANY(g_active))) {
        int au = 1;                                              // uniform copy of `a`
        while (au < a_end) {
            if (au >= 2 && au < S2K_ADDS_P && !(au & 1)) {
#pragma unroll 1
                for (int k = 0; k < 4; k++) gej_double_lean(R, R);
                S2K_PROF_MARK(6);
            }
            if (au == S2K_ADD_G0) { fe zi; ptab_load_ziso(zi, ptab); fe_mul(R.z, R.z, zi); zfixed = 1; }      // back to the real curve
#pragma unroll
            for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];                  // request the next record before the arithmetic
            gej t; const int same_x = gej_add_ge_lean(t, R, cur);
            if (S2K_WAVE_ANY(same_x & cur_valid)) break;                        // -> general loop, nothing committed
            if (au < S2K_ADDS_P) R = t;                                         // regular digits are never zero
            else if (cur_valid) R = t;                                          // generator windows: a zero window adds nothing (per lane)
            au++;
            op_decode(cur, raw, nxt_neg, nxt_lam); cur_valid = nxt_valid;
            op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, au + 1);
        }
        if (au == S2K_ADD_G0 && !zfixed) { fe zi; ptab_load_ziso(zi, ptab); fe_mul(R.z, R.z, zi); zfixed = 1; }      // no generator part
        a = au;
    }
#endif
    int done = !(a < a_end) & zfixed;
    while (S2K_WAVE_ANY(!done)) {
        int do_dbl = 0, do_add = 0;
        if (!done) {
            if (pending) { do_dbl = 1; pending = 0; }
            else if (dbl_left > 0) { do_dbl = !R.inf; dbl_left--; }
            else do_add = 1;
        }
        if (S2K_WAVE_ANY(do_dbl)) {
            gej t; gej_double(t, R);
            if (do_dbl) R = t;
        }
        if (S2K_WAVE_ANY(do_add)) {
#pragma unroll
            for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];                  // request the next record before the arithmetic
            gej t; const int f = gej_add_ge(t, R, cur);
            ge nx; op_decode(nx, raw, nxt_neg, nxt_lam);
            if (do_add) {
                if (cur_valid) { R = t; pending = (f == GEJ_ADD_NEEDS_DOUBLE); }
                a++;
                cur = nx; cur_valid = nxt_valid;
                dbl_left = (a >= 2 && a < S2K_ADDS_P && !(a & 1)) ? 4 : 0;
                op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, a + 1);
            }
        }
        // leaving the isomorphic curve: after the last digit, before the generator additions
        const int fix = (!done) & (!zfixed) & (a == S2K_ADD_G0) & (!pending);
        if (S2K_WAVE_ANY(fix)) {
            fe zi;
#pragma unroll
            for (int i = 0; i < 9; i++) zi.n[i] = ptab[S2K_PTAB_ZISO + i];
            fe z; fe_mul(z, R.z, zi);
            if (fix) { R.z = z; zfixed = 1; }
        }
        if ((a >= a_end) & (!pending) & zfixed) done = 1;
    }
    S2K_PROF_MARK(3);
}


// ---- the same multiplication with the variable part cut in two: R = na*A + ng*G given also T = 2^64 * A -------------------------
// When 2^64*A is known (the rangeproof rings keep it next to every ring key: one 64-doubling chain per ring, then the same
// "+ base" step as the key itself, rangeproof.h), each odd GLV half k = ka + 2^64 kb splits into two 65-bit odd pieces and
//     na*A = (+-k1a) A + (+-k2a) lambda A + (+-k1b) T + (+-k2b) lambda T
// needs 64 doublings instead of 128, for one more table and two more additions: four digit streams of 17 signed odd 4-bit
// digits, 4 doublings + 4 additions per digit position.  Both tables are rescaled to ONE common Z (ptab_rescale), so the
// accumulator sits on one isomorphic curve as before.  Only the lock-step form exists: the function returns 0 without having
// produced anything when the wavefront is not uniform or a lane meets an operand with its own x coordinate, and the caller then
// runs ecmult_lane.  Digit stream in LDS: words 0..7 = nibble (pos * 4 + stream), words 8..16 = ng recoded (gtab_recode).
#define S2K_SPLIT_ADDS_P 68          // 4 streams x 17 digits
struct piece65 { u32 w[3]; int neg; };
S2K_HD void sc_split_pieces(piece65 out[4], const half_scalar& h0, const half_scalar& h1) {
    // out[0] = low piece of k1, out[1] = low piece of k2, out[2] = high piece of k1, out[3] = high piece of k2 (stream order)
    for (int hf = 0; hf < 2; hf++) {
        const half_scalar& h = hf ? h1 : h0;
        u32 lo[3] = {h.w[0], h.w[1], 0u};
        u32 hi[3] = {h.w[2], h.w[3], h.w[4]};                        // k >> 64 (< 2^65)
        int lo_neg = h.neg;
        if (!(hi[0] & 1u)) {                                         // make the high piece odd: hi += 1, lo -= 2^64 (lo becomes negative)
            u32 c = 1u;
            for (int i = 0; i < 3; i++) { const u32 t = hi[i] + c; c = (t < c); hi[i] = t; }
            // |lo - 2^64| = 2^64 - lo  (lo odd, so nonzero)
            const u64 l = (u64)lo[0] | ((u64)lo[1] << 32);
            const u64 m = 0ull - l;
            lo[0] = (u32)m; lo[1] = (u32)(m >> 32); lo[2] = 0u;
            lo_neg = !h.neg;
        }
        for (int i = 0; i < 3; i++) { out[hf].w[i] = lo[i]; out[2 + hf].w[i] = hi[i]; }
        out[hf].neg = lo_neg; out[2 + hf].neg = h.neg;
    }
}
S2K_HD int ecmult_lane_split(gej& R, const gej& A, const gej& T, const scalar& na, const scalar& ng, int has_ng, const u32* gtab, const lane_mem& lm) {
    u32* const ptab = lm.ptab; const s2k_lds_ptr dig = lm.dig;
    const int p_active = (!A.inf) & (!T.inf) & (!sc_is_zero(na));
    const int g_active = has_ng & (!sc_is_zero(ng));
    if (!(S2K_WAVE_ALL(p_active) && (S2K_WAVE_ALL(g_active) || !S2K_WAVE_ANY(g_active)))) return 0;
    u32 sneg = 0;                                                    // bit st: stream st is negative
    S2K_PROF_DECL;
    {
        half_scalar h0, h1; sc_split_lambda_odd(h0, h1, na);
        piece65 pc[4]; sc_split_pieces(pc, h0, h1);
        u32 dw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) dw[i] = 0;
#pragma unroll
        for (int st = 0; st < 4; st++) {
            sneg |= (u32)pc[st].neg << st;
#pragma unroll
            for (int pos = 0; pos < 16; pos++) {                     // pos 0 = digit 15 (most significant after the fixed top digit)
                const int i = 15 - pos, bit = 4 * i + 1, word = bit >> 5, sh = bit & 31;
                const u64 pair = (u64)pc[st].w[word] | ((u64)(word + 1 < 3 ? pc[st].w[word + 1] : 0u) << 32);
                const u32 v = (u32)(pair >> sh) & 15u;
                const int nib = pos * 4 + st;
                dw[nib >> 3] |= v << ((nib & 7) * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) dig[i * S2K_DIG_STRIDE] = dw[i];
        {
            u32 ngr[S2K_GTAB_SWORDS]; gtab_recode(ngr, ng.d, gtab);
#pragma unroll
            for (int i = 0; i < S2K_GTAB_SWORDS; i++) dig[(8 + i) * S2K_DIG_STRIDE] = ngr[i];
        }
        fe za, zt, ziso;
        S2K_PROF_MARK(1);
        ptab_build_raw(za, ptab, A);
        ptab_build_raw(zt, ptab + S2K_PTAB_TABLE_WORDS, T);
        S2K_PROF_MARK(8);
        ptab_rescale(ptab, &zt);
        ptab_rescale(ptab + S2K_PTAB_TABLE_WORDS, &za);
        S2K_PROF_MARK(9);
        fe_mul(ziso, za, zt);
#pragma unroll
        for (int i = 0; i < 9; i++) ptab[S2K_PTAB_ZISO + i] = ziso.n[i];
    }
    const gtab_geom GG = gtab_geometry(gtab);
    const int a_g0 = S2K_SPLIT_ADDS_P;
    const int a_end = g_active ? a_g0 + (int)GG.W : a_g0;
    auto op_locate = [&](const u32*& addr, int& valid, int& neg, int& lam, int idx) {
        addr = ptab; valid = 0; neg = 0; lam = 0;
        if (idx < a_g0) {
            const int st = idx & 3;
            u32 v = 8u;                                                                     // the fixed top digit +1
            if (idx >= 4) { const int nib = idx - 4; v = (dig[(nib >> 3) * S2K_DIG_STRIDE] >> ((nib & 7) * 4)) & 15u; }
            valid = 1;
            neg = (v < 8u) ^ (int)((sneg >> st) & 1u);
            const u32 e = (v < 8u) ? (7u - v) : (v - 8u);
            addr = ptab + (st >> 1) * S2K_PTAB_TABLE_WORDS + e * S2K_PTAB_ENTRY_WORDS + (((st & 1) && S2K_PTAB_TWINS) ? 16 : 0); lam = (st & 1) && !S2K_PTAB_TWINS;
        } else if (idx < a_end) {
            const int g = idx - a_g0, w = (int)(((u32)g * GG.D) >> 5);
            valid = gtab_locate(addr, neg, gtab, GG, g, dig[(8 + w) * S2K_DIG_STRIDE], w + 1 < S2K_GTAB_SWORDS ? dig[(9 + w) * S2K_DIG_STRIDE] : 0u);
        }
    };
    auto op_decode = [&](ge& o, const u32 raw[16], int neg, int lam) {
        fe y, yn;
        fe_from_words(o.x, raw); fe_from_words(y, raw + 8);
        if (lam) { fe beta; fe_set_beta(beta); fe_mul(o.x, o.x, beta); }          // `lam` is a compile-time constant at every call site
        fe_neg(yn, y, 1);
        fe_select(o.y, yn, y, neg);
    };
    const u32* nxt_addr; int nxt_valid, nxt_neg, nxt_lam;
    u32 raw[16];
    ge cur; int cur_valid;
    op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, 0);
#pragma unroll
    for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
    op_decode(cur, raw, nxt_neg, 0);
    op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, 1);
    // Variable part: additions 0..67 as 34 (plain stream, lambda stream) pairs -- the trip holds both additions, so which operand
    // takes the beta product is static and the accumulator can alternate between two register sets instead of being copied back at
    // every loop edge.  Addition 0 adds to infinity: it just takes its operand.  In place: a lane that meets its own x coordinate
    // makes the caller start over with ecmult_lane, so the accumulator of before the addition need not survive it.
    int au = 0;
    while (au < a_g0) {
        if (au >= 4 && !(au & 3)) {
#pragma unroll 1
            for (int k = 0; k < 4; k++) gej_double_lean(R, R);
            S2K_PROF_MARK(6);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];                  // request the next record before the arithmetic
        if (au == 0) gej_set_ge(R, cur);
        else { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        op_decode(cur, raw, nxt_neg, !S2K_PTAB_TWINS);                      // operand of the lambda stream
        op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, au + 2);           // (au = 66: the first generator window, if any)
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
        { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        au += 2;
        op_decode(cur, raw, nxt_neg, 0); cur_valid = nxt_valid;
        op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, au + 1);
    }
    { fe zi; ptab_load_ziso(zi, ptab); fe_mul(R.z, R.z, zi); }             // back to the real curve
    // generator part: a zero window adds nothing (per lane), so these additions are committed by select
#if S2K_XYZZ_TABLE_PART
    gez acc4; acc4.inf = 0; acc4.x = R.x; acc4.y = R.y;
    fe_sqr(acc4.zz, R.z); fe_mul(acc4.zzz, acc4.zz, R.z);
#endif
    while (au < a_end) {
#if S2K_NT_GTAB_SPLIT && defined(__HIP_DEVICE_COMPILE__)
        {   // (the fixed-base operands are touched once: a non-temporal request keeps them from displacing the per-lane tables)
            typedef unsigned int s2k_u32x4 __attribute__((ext_vector_type(4)));
            const s2k_u32x4* q = (const s2k_u32x4*)nxt_addr;
#pragma unroll
            for (int k = 0; k < 4; k++) { const s2k_u32x4 v = __builtin_nontemporal_load(q + k); raw[4 * k] = v.x; raw[4 * k + 1] = v.y; raw[4 * k + 2] = v.z; raw[4 * k + 3] = v.w; }
        }
#else
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
#endif
#if S2K_XYZZ_TABLE_PART
        {
            gez t = acc4; gez_add_ge_lean(t, cur);
            if (S2K_WAVE_ALL(cur_valid)) acc4 = t;               // (a zero digit -- one window value in 2^D -- is the only reason for the selects)
            else { fe_cmov(acc4.x, t.x, cur_valid); fe_cmov(acc4.y, t.y, cur_valid); fe_cmov(acc4.zz, t.zz, cur_valid); fe_cmov(acc4.zzz, t.zzz, cur_valid); }
        }
#else
        gej t; const int same_x = gej_add_ge_lean(t, R, cur);
        if (S2K_WAVE_ANY(same_x & cur_valid)) return 0;
        if (cur_valid) R = t;
#endif
        au++;
        op_decode(cur, raw, nxt_neg, nxt_lam); cur_valid = nxt_valid;
        op_locate(nxt_addr, nxt_valid, nxt_neg, nxt_lam, au + 1);
    }
#if S2K_XYZZ_TABLE_PART
    if (S2K_WAVE_ANY(fe_normalizes_to_zero(acc4.zz))) return 0;
    gej_set_gez(R, acc4);
#endif
    S2K_PROF_MARK(10);
#ifdef S2K_ON_SPLIT_DONE
    S2K_ON_SPLIT_DONE();                                                                      // host test build: count completed split runs
#endif
    return 1;
}


// ---- the ring form: several multiplications by the SAME point  R_j = e_j*C + s_j*G + f_j*H ---------------------------------------
// A Borromean ring verifies four public keys P_j = C + j*B with B = -(4^i 10^exp)*H a known multiple of the proof's generator H
// (secp256k1_rangeproof_pub_expand, rangeproof_impl.h:19-51), so   e_j*P_j = e_j*C + f_j*H ,  f_j = -(j 4^i 10^exp) e_j mod n :
// the variable point is the same for all four steps of the ring, and the part that changes goes through a fixed-base table of H laid
// out exactly like the one of G (gtable.h; the engine keeps a small cache of them keyed by the generator's 64 bytes).  What that buys:
//   * the table of the variable point and the 64-doubling chain to T = 2^64*C are built ONCE per ring instead of once per step, so the
//     table can be twice as large as ecmult_lane_split's two: 32 sectors of 64 bytes;
//   * no "key <- key + B", "T <- T + 2^64*B" updates between the steps;
//   * + W (the table's number of windows) additions from H's table on the steps with j > 0.
// What the rangeproof rings run is the six-base form further down (ecmult_ring6_tables / ecmult_ring6_step, S2K_RING_SIX in rangeproof.h), over
// the three bases of the three-base form (ecmult_ring3_tables / ecmult_ring3_step, S2K_RING_TRIPLE) and their lambda images; both share the
// step body, the sizes and the digit-word layout with the joint form described here, and the two older forms stay for A/B runs.
// The joint form (S2K_RING_JOINT = 1, the default): ONE table indexed by the digits of BOTH bases.  Its 32 sectors hold
//     J(a, b) = a*C + b*T ,  a in {1, 3, 5, 7},  b in {+-1, +-3, +-5, +-7} ,  at sector ((a - 1) / 2) * 8 + (b + 7) / 2 ,
// all on one Z, and a plain operand carries the digit of the C piece and the digit of the T piece of a GLV half at once (the lambda
// operand is the same entry with beta on x).  The four 65-bit pieces of sc_split_pieces are odd and below 2^65; each is cut into 22 signed
// odd 3-bit digits d_i = 2 b_i - 7, and 22 of them need no fixed top digit: sum d_i 8^i = 2B - (2^66 - 1), so b is read off
// B = (k - 1)/2 + 2^65 -- bit t of B is bit t + 1 of k, bit 64 is clear and bit 65 set, i.e. the top field is 4 | bit 63 of B.  With the
// pieces' signs folded in, level i of a half has the signed digits (dC, dT) and takes  sign(dC) * J(|dC|, sign(dC) dT) : an entry index and
// ONE negation flag (ring_joint_field), six bits.
// A step is 22 levels (3 doublings in front of every level but the first; plain operand, lambda operand): 63 doublings and 44 additions,
// the first of which just takes its operand, and 22 beta products.
// Per ring: 1 chain + the table + 4 x (63 doublings + 44 additions) + 77 table additions, against 4 x (64 doublings + 68 + 11 additions
// + 2 tables + a chain quarter + 2 key updates) for ecmult_lane_split.
// Construction (ecmult_ring_tables): two 4-entry chains of odd multiples (ptab_build_raw_n<4>), both rescaled to one Z; 16 conjugate
// additions (aC + bT and aC - bT together: Z = dx for both, 5M + 3S the pair); then every pair is brought to the product of all sixteen dx
// by prefix / suffix products.  370 products + squarings per ring.  No addition in it can be exceptional for a finite C (a*C = +-b*T would
// need n | a -+ b 2^64: odd, nonzero, below n); a dx of zero would all the same end up as a factor of the Z factor, and a step that finds
// the Z factor zero returns 0 like one that met an exceptional addition.
// Lane memory: `rtab`, S2K_RTAB_WORDS words of HBM: 32 finished 64-byte sectors back to back (2 KB: all the main loop touches) and the Z
// factor; the parked entries of the construction live in a per-wavefront, lane-interleaved area (S2K_RRAW_WAVE_WORDS).  A lane's 32 x 27
// words of it (word w at raw[w * S2K_RAW_WS]) during the construction:
//     words   0..143  the eight rescaled chain entries, 18 words (x, y) each: 0..3 = C, 3C, 5C, 7C; 4..7 = T, 3T, 5T, 7T
//     words 144..863  pair k = 4 * ((a - 1) / 2) + (b - 1) / 2 : 45 words (x+, y+, x-, y-, product of the dx before it)
//     (slots 24..31, i.e. words 648..863, first hold the two chains as ptab_build_raw_n parks them; they are dead before pair 11 is written)
// Digit stream in LDS (S2K_RING_DIG_WORDS words per lane): words 0..8 = six-bit field (level * 2 + half), five per word; 9..17 = s and
// 18..26 = f, both recoded for the signed fixed-base windows (gtab_recode).
// Only the lock-step form exists (every lane of the wavefront works: the caller gives idle lanes a dummy point and dummy scalars);
// ecmult_ring_step returns 0, having produced nothing, when a lane met an operand with its own x coordinate, and the caller then takes
// that step through ecmult_lane on P_j itself.
//
// The separate form (S2K_RING_JOINT = 0: what the joint form replaced, kept for A/B runs and as the control of the host tests): two
// 16-entry tables of odd multiples, of C and of T, one operand per piece.  Signed odd 5-bit digits, 13 additions per stream
// (13, not 14: 13 digits d_i = 2 b_i - 31 represent every odd k with |k| < 2^65 -- sum d_i 32^i = 2B - (2^65 - 1), so b is read off
// B = (k - 1)/2 + 2^64: bit t of B is bit t + 1 of k and bit 64 is set, i.e. the top digit is 16 | (k >> 61).  ecmult_lane_split's 4-bit
// digits need a fixed 17th digit because 16 of them only reach 2^64.)  So a step is 12 x 5 doublings, 52 additions and 26 beta products;
// the construction is two chains of one doubling + 15 co-Z additions and 32 rescales, 385 products + squarings per ring.  Digit words
// 0..8 = 5-bit digit (pos * 4 + stream), six per word.
#ifndef S2K_RING_JOINT
#define S2K_RING_JOINT 1
#endif
#if S2K_RING_JOINT
#define S2K_RING_W 3
#define S2K_RING_DIGITS 22                                      /* 22 signed odd 3-bit digits: every odd |k| < 2^66, no extra top digit */
#define S2K_RING_ADDS_P (2 * S2K_RING_DIGITS)                   /* one operand per level and GLV half */
#define S2K_RING_GROUP 2                                        /* additions between two runs of doublings */
#else
#define S2K_RING_W 5
#define S2K_RING_DIGITS 13                                      /* 13 signed odd 5-bit digits: every odd |k| < 2^65, no extra top digit (below) */
#define S2K_RING_ADDS_P (4 * S2K_RING_DIGITS)
#define S2K_RING_GROUP 4
#endif
#define S2K_RING_ENTRIES 16                                     /* (per table in the separate form; the joint table has 2 x 16 sectors) */
#define S2K_RING_DIG_WORDS 27
#define S2K_RTAB_TABLE_WORDS (S2K_RING_ENTRIES * 16)
#define S2K_RTAB_ZISO (2 * S2K_RTAB_TABLE_WORDS)
#define S2K_RTAB_WORDS (S2K_RTAB_ZISO + 16)                     /* per lane: 32 finished sectors + the Z factor */
// parking area of the construction: per WAVEFRONT, word k of parked entry e of the 64 lanes at ((e * 27 + k) * 64 + lane)
#if defined(__HIP_DEVICE_COMPILE__)
#define S2K_RAW_WS 64
#else
#define S2K_RAW_WS 1
#endif
#define S2K_RAW_ES (27 * S2K_RAW_WS)
#define S2K_RRAW_WAVE_WORDS (2 * S2K_RING_ENTRIES * 27 * 64)

// word w .. w + 8 of this lane's column of the parking area
S2K_HD void rraw_store(u32* raw, int w, const fe& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        if (S2K_NT_PARK && S2K_RAW_WS > 1) S2K_ST_NT(a.n[i], &raw[(w + i) * S2K_RAW_WS]);
        else raw[(w + i) * S2K_RAW_WS] = a.n[i];
    }
}
S2K_HD void rraw_load(fe& a, const u32* raw, int w) {
#pragma unroll
    for (int i = 0; i < 9; i++) a.n[i] = (S2K_NT_PARK && S2K_RAW_WS > 1) ? S2K_LD_NT(&raw[(w + i) * S2K_RAW_WS]) : raw[(w + i) * S2K_RAW_WS];
}
#if S2K_RING_JOINT
#define S2K_RJ_CHAIN_SLOT 24                                    /* the two raw chains: slots 24..27 (C) and 28..31 (T) of the parking area */
#define S2K_RJ_PAIR0 144                                        /* first word of pair 0 */
#define S2K_RJ_PAIR_WORDS 45
// the 3-bit field b_i (digit d_i = 2 b_i - 7, i = 0 least significant) of an odd piece below 2^65
S2K_HD u32 ring_piece_field(const piece65& p, int i) {
    const int bit = S2K_RING_W * i + 1, word = bit >> 5, sh = bit & 31;
    const u64 pair = (u64)p.w[word] | ((u64)(word + 1 < 3 ? p.w[word + 1] : 0u) << 32);
    u32 v = (u32)(pair >> sh) & 7u;
    if (i == S2K_RING_DIGITS - 1) v |= 4u;                      // bit 65 of B (the piece is below 2^65: bits 65, 66 of it are clear)
    return v;
}
// fields vc, vt of the C piece and the T piece at one level, sc, st the pieces' signs (1 = negative)  ->  neg << 5 | sector: the operand is
// sign(dC) * J(|dC|, sign(dC) * dT) with dC = +-(2 vc - 7), dT = +-(2 vt - 7)
S2K_HD u32 ring_joint_field(u32 vc, u32 vt, u32 sc, u32 st) {
    const u32 neg = (u32)(vc < 4u) ^ sc;
    const u32 ai = vc < 4u ? 3u - vc : vc - 4u;                 // (|dC| - 1) / 2
    const u32 bi = vt ^ ((neg ^ st) ? 7u : 0u);                 // (b + 7) / 2 ; negating b = 2 vt - 7 is vt -> 7 - vt
    return (neg << 5) | (ai << 3) | bi;
}
// the digit words 0..8 of a step: field (level * 2 + half), level 0 = most significant, five six-bit fields per word
S2K_HD void ring_joint_recode(u32 dw[9], const piece65 pc[4]) {
#pragma unroll
    for (int i = 0; i < 9; i++) dw[i] = 0;
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
#pragma unroll
        for (int pos = 0; pos < S2K_RING_DIGITS; pos++) {
            const int i = S2K_RING_DIGITS - 1 - pos, idx = pos * 2 + hf;
            const u32 v = ring_joint_field(ring_piece_field(pc[hf], i), ring_piece_field(pc[2 + hf], i), (u32)pc[hf].neg, (u32)pc[2 + hf].neg);
            dw[idx / 5] |= v << ((idx % 5) * 6);
        }
    }
}
// C, T = 2^64*C finite, magnitudes <= (5,3,1).  rtab: this lane's S2K_RTAB_WORDS; raw: this lane's column of its wavefront's parking area
S2K_HD void ecmult_ring_tables(u32* rtab, u32* raw, const gej& C, const gej& T) {
    {   // the chains, both on the Z  za * zt  (which waits in the Z factor's place)
        fe za, zt, zs;
        ptab_build_raw_n<4, S2K_RAW_WS, S2K_RAW_ES>(za, raw + S2K_RJ_CHAIN_SLOT * S2K_RAW_ES, C);
        ptab_build_raw_n<4, S2K_RAW_WS, S2K_RAW_ES>(zt, raw + (S2K_RJ_CHAIN_SLOT + 4) * S2K_RAW_ES, T);
#pragma unroll 1
        for (int e = 7; e >= 0; e--) {
            if ((e & 3) == 3) zs = (e >> 2) ? za : zt;          // each chain by the OTHER one's Z
            fe x, y, h, zs2, zs3;
            rraw_load(x, raw, (S2K_RJ_CHAIN_SLOT + e) * 27); rraw_load(y, raw, (S2K_RJ_CHAIN_SLOT + e) * 27 + 9); rraw_load(h, raw, (S2K_RJ_CHAIN_SLOT + e) * 27 + 18);
            fe_sqr(zs2, zs); fe_mul(zs3, zs2, zs);
            fe_mul2(x, x, zs2, y, y, zs3);
            rraw_store(raw, 18 * e, x); rraw_store(raw, 18 * e + 9, y);
            fe_mul(zs, zs, h);                                  // ratio z_i / z_{i-1} joins the running product for the entries below
        }
        fe_mul(zs, za, zt);
#pragma unroll
        for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = zs.n[i];
    }
    {   // the pairs: P1 = aC, P2 = bT as affine points of the chains' curve; P1 + P2 and P1 - P2 both come out with Z = dx = x2 - x1
        fe p; fe_set_int(p, 1);
#pragma unroll 1
        for (int k = 0; k < 16; k++) {
            const int w1o = 18 * (k >> 2), w2o = 18 * (4 + (k & 3)), rec = S2K_RJ_PAIR0 + S2K_RJ_PAIR_WORDS * k;
            fe x1, y1, x2, y2;
            rraw_load(x1, raw, w1o); rraw_load(y1, raw, w1o + 9); rraw_load(x2, raw, w2o); rraw_load(y2, raw, w2o + 9);
            fe dx, dy, sy, t, c, d, d2, w1, w2, e, a1, x3, x3m, y3, y3m;
            fe_neg(t, x1, 1); fe_add2(dx, x2, t); fe_norm_weak(dx);
            fe_neg(t, y1, 1); fe_add2(dy, y2, t); fe_norm_weak(dy);
            fe_add2(sy, y1, y2); fe_norm_weak(sy);
            fe_sqr2(c, dx, d, dy);
            fe_mul2(w1, x1, c, w2, x2, c);
            fe_neg(e, w1, 1); fe_add(e, w2);                                  // dx^3                        (3)
            fe_mul_sqr(a1, y1, e, d2, sy);                                    // (1*3)
            fe_add2(t, w1, w2); fe_neg(t, t, 2);                              // -(W1 + W2)                  (3)
            fe_add2(x3, d, t); fe_add2(x3m, d2, t);                           // X(P1 + P2), X(P1 - P2)      (4)
            fe_neg(t, x3, 4); fe_add(t, w1);                                  // W1 - X3                     (6)
            fe_neg(e, w1, 1); fe_add(e, x3m);                                 // X3' - W1                    (6)
            fe_mul2(y3, dy, t, y3m, sy, e);                                   // (1*6, 1*6)
            fe_neg(t, a1, 1); fe_add(y3, t); fe_add(y3m, t);                  // Y = dy (W1 - X3) - y1 dx^3 ; Y' = sy (X3' - W1) - y1 dx^3   (3)
            rraw_store(raw, rec, x3); rraw_store(raw, rec + 9, y3); rraw_store(raw, rec + 18, x3m); rraw_store(raw, rec + 27, y3m);
            rraw_store(raw, rec + 36, p);
            fe_mul(p, p, dx);
        }
    }
    fe s; fe_set_int(s, 1);
#pragma unroll 1
    for (int k = 15; k >= 0; k--) {                              // pair k times (product of the other fifteen dx): every entry on Z = za zt prod dx
        const int ai = k >> 2, bi = k & 3, rec = S2K_RJ_PAIR0 + S2K_RJ_PAIR_WORDS * k;
        fe xp, yp, xm, ym, m, x1, dx;
        rraw_load(xp, raw, rec); rraw_load(yp, raw, rec + 9); rraw_load(xm, raw, rec + 18); rraw_load(ym, raw, rec + 27); rraw_load(m, raw, rec + 36);
        rraw_load(x1, raw, 18 * ai); rraw_load(dx, raw, 18 * (4 + bi));
        fe_neg(x1, x1, 1); fe_add(dx, x1); fe_norm_weak(dx);
        fe_mul2(m, m, s, s, s, dx);
        fe m2, m3; fe_sqr(m2, m); fe_mul(m3, m2, m);
        fe_mul2(xp, xp, m2, xm, xm, m2);                                      // (4*1)
        fe_mul2(yp, yp, m3, ym, ym, m3);                                      // (3*1)
        fe_normalize(xp); fe_normalize(yp); fe_normalize(xm); fe_normalize(ym);
        u32* const ep = rtab + (ai * 8 + 4 + bi) * 16;                        // J(a, +b)
        u32* const em = rtab + (ai * 8 + 3 - bi) * 16;                        // J(a, -b)
        u32 wx[8], wy[8];
        fe_to_words(wx, xp); fe_to_words(wy, yp);
#pragma unroll
        for (int i = 0; i < 8; i++) { ep[i] = wx[i]; ep[8 + i] = wy[i]; }
        fe_to_words(wx, xm); fe_to_words(wy, ym);
#pragma unroll
        for (int i = 0; i < 8; i++) { em[i] = wx[i]; em[8 + i] = wy[i]; }
    }
    fe ziso;
#pragma unroll
    for (int i = 0; i < 9; i++) ziso.n[i] = rtab[S2K_RTAB_ZISO + i];
    fe_mul(ziso, ziso, s);                                                    // (a dx of zero makes the Z factor zero: ecmult_ring_step then returns 0)
#pragma unroll
    for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = ziso.n[i];
}
#else
S2K_HD void ecmult_ring_tables(u32* rtab, u32* raw, const gej& C, const gej& T) {
    fe za, zt, ziso;
    u32* const raw_t = raw + S2K_RING_ENTRIES * S2K_RAW_ES;
    ptab_build_raw_n<S2K_RING_ENTRIES, S2K_RAW_WS, S2K_RAW_ES>(za, raw, C);
    ptab_build_raw_n<S2K_RING_ENTRIES, S2K_RAW_WS, S2K_RAW_ES>(zt, raw_t, T);
    ptab_rescale_n<S2K_RING_ENTRIES, S2K_RAW_WS, S2K_RAW_ES>(raw, rtab, 16, &zt);
    ptab_rescale_n<S2K_RING_ENTRIES, S2K_RAW_WS, S2K_RAW_ES>(raw_t, rtab + S2K_RTAB_TABLE_WORDS, 16, &za);
    fe_mul(ziso, za, zt);
#pragma unroll
    for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = ziso.n[i];
}
#endif
// ---- the three-base form of the ring table (S2K_RING_TRIPLE, rangeproof.h) -------------------------------------------------------
// Every odd GLV half k < 2^129 is cut into THREE 43-bit pieces, k = p0 + 2^43 p1 + 2^86 p2, over the bases C, T1 = 2^43*C and T2 = 2^86*C.
// From the top down each piece is made odd by the borrow of sc_split_pieces (+1 on it, -2^43 on the piece below it), so a piece carries
// its own sign and every magnitude is odd and below 2^43.  A piece becomes 22 signed odd 2-bit digits d_i = 2 b_i - 3:
// sum d_i 4^i = 2B - (2^44 - 1), so b is read off B = (v - 1)/2 + 2^43 -- bit t of B is bit t + 1 of v and bit 43 is set -- which represents
// every odd v <= 2^44 - 1 with no fixed top digit.  Level i of a half has the signed digits (dC, d1, d2) in {+-1, +-3}^3 and takes
//     sign(dC) * J(|dC|, sign(dC) d1, sign(dC) d2) ,   J(a, b, c) = a*C + b*T1 + c*T2 ,  a in {1, 3},  b, c in {+-1, +-3} ,
// at sector ((a - 1) / 2) * 16 + ((b + 3) / 2) * 4 + (c + 3) / 2: the same 32 sectors, and the same six-bit field neg << 5 | sector at
// the same place (level * 2 + half, five per word) that ecmult_ring_step's operand lookup reads for the joint form.
// A step is 22 levels of 2 doublings (none in front of the first) + 2 additions: 42 doublings, 44 additions, 22 beta products; the
// chain is 86 doublings per ring instead of 64.
// Construction (ecmult_ring3_tables): three 2-entry chains {P, 3P} of C, T1 and T2 (ptab_build_raw_n<2>) rescaled to one Z (za z1 z2);
// stage 1: the four conjugate pairs b*T1 +- c*T2 (b, c in {1, 3}), brought to the product D1 of their four dx, which gives the eight
// Q = b*T1 + c*T2 with b > 0 (q = 4 (b - 1)/2 + 2 (|c| - 1)/2 + (c < 0)), and C, 3C rescaled by D1; stage 2: the sixteen conjugate
// pairs a*C +- Q (pair k = 8 (a - 1)/2 + q: a*C + Q = J(a, b, c), a*C - Q = J(a, -b, -c)), brought to the product D2 of their sixteen dx
// by prefix / suffix products and packed.  The Z factor is za z1 z2 D1 D2.  No addition in it can be exceptional for a finite C (a
// coincidence needs n to divide a small nonzero odd combination of 1, 2^43 and 2^86); a dx of zero ends up as a factor of the Z factor
// all the same, and a step that finds the Z factor zero returns 0.
// The sums of a pair are never parked: Z = dx of a pair is a difference of two parked inputs, so a first pass forms the prefix products of
// the dx from the inputs alone and the second adds each pair once, in registers (ring3_pair_batch).
// A lane's words of the parking area (word w at raw[w * S2K_RAW_WS]) during the construction -- W = 414 of the 32 x 27 are used, 612 are
// written per ring (162 + 108 + 27 + 144 + 36 + 135):
//     words   0..35   C, 3C, 18 words (x, y) each: on the chains' Z, then on D1
//     words  36..179  Q_0..Q_7, 18 words each (written by the second pass of stage 1)
//     words 180..314  stage 2: the product of the dx before pair k, k = 1..15, 9 words each at 180 + 9 (k - 1) (that of pair 0 is 1)
//     before stage 2 the same words hold: 180..251 T1, 3T1, T2, 3T2 (18 words each, rescaled), 252..278 stage 1's three prefix products,
//     and before stage 1 252..413 the three chains as ptab_build_raw_n parks them (6 slots of 27 words)
//     words 414..863  unused by this form (the joint form, which shares the area's size, uses all 864)
struct piece43 { u64 m; int neg; };
#define S2K_R3_DIGITS 22
#define S2K_R3_Q0 36
#define S2K_R3_PROD0 180
#define S2K_R3_T0 180
#define S2K_R3_S1PROD0 252
#define S2K_R3_CHAIN0 252
#define S2K_R3_PARK_WORDS 414                                   /* W: the highest used word + 1 */
#ifndef S2K_R3_AHEAD
#define S2K_R3_AHEAD 1
#endif
// out[0], out[1] = C pieces of k1, k2; out[2], out[3] = T1 pieces; out[4], out[5] = T2 pieces (sign of the half folded in)
S2K_HD void sc_split_pieces3(piece43 out[6], const half_scalar& h0, const half_scalar& h1) {
    const u64 mask = (1ull << 43) - 1ull;
    for (int hf = 0; hf < 2; hf++) {
        const half_scalar& h = hf ? h1 : h0;
        const u64 lo = (u64)h.w[0] | ((u64)h.w[1] << 32), mid = (u64)h.w[2] | ((u64)h.w[3] << 32);
        long long p0 = (long long)(lo & mask);
        long long p1 = (long long)(((lo >> 43) | (mid << 21)) & mask);
        long long p2 = (long long)((mid >> 22) | ((u64)h.w[4] << 42));            // k >> 86 (< 2^43)
        if (!(p2 & 1)) { p2 += 1; p1 -= (long long)(1ull << 43); }                // top piece odd: +1 on it, -2^43 on the one below
        if (!(p1 & 1)) { p1 += 1; p0 -= (long long)(1ull << 43); }                // (p0 is odd as k is: p0 - 2^43 is odd and nonzero)
        const long long p[3] = {p0, p1, p2};
        for (int b = 0; b < 3; b++) { out[2 * b + hf].m = (u64)(p[b] < 0 ? -p[b] : p[b]); out[2 * b + hf].neg = (p[b] < 0) ^ h.neg; }
    }
}
// the 2-bit field b_i (digit d_i = 2 b_i - 3, i = 0 least significant) of an odd piece magnitude <= 2^44 - 1
S2K_HD u32 ring3_piece_field(u64 m, int i) { return (u32)((((m >> 1) | (1ull << 43)) >> (2 * i)) & 3ull); }
// fields vc, v1, v2 of the pieces on C, T1, T2 at one level, sc, s1, s2 their signs (1 = negative)  ->  neg << 5 | sector
S2K_HD u32 ring3_field(u32 vc, u32 v1, u32 v2, u32 sc, u32 s1, u32 s2) {
    const u32 neg = (u32)(vc < 2u) ^ sc;
    const u32 ai = vc < 2u ? 1u - vc : vc - 2u;                 // (|dC| - 1) / 2
    const u32 bi = v1 ^ ((neg ^ s1) ? 3u : 0u);                 // (b + 3) / 2 ; negating b = 2 v - 3 is v -> 3 - v
    const u32 ci = v2 ^ ((neg ^ s2) ? 3u : 0u);
    return (neg << 5) | (ai << 4) | (bi << 2) | ci;
}
// the digit words 0..8 of a step: field (level * 2 + half), level 0 = most significant, five six-bit fields per word
S2K_HD void ring3_recode(u32 dw[9], const piece43 pc[6]) {
#pragma unroll
    for (int i = 0; i < 9; i++) dw[i] = 0;
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
#pragma unroll
        for (int pos = 0; pos < S2K_R3_DIGITS; pos++) {
            const int i = S2K_R3_DIGITS - 1 - pos, idx = pos * 2 + hf;
            const u32 v = ring3_field(ring3_piece_field(pc[hf].m, i), ring3_piece_field(pc[2 + hf].m, i), ring3_piece_field(pc[4 + hf].m, i),
                                      (u32)pc[hf].neg, (u32)pc[2 + hf].neg, (u32)pc[4 + hf].neg);
            dw[idx / 5] |= v << ((idx % 5) * 6);
        }
    }
}
// One batch of N conjugate pairs P1 +- P2 (both affine on one curve: 18 parked words (x, y) each, pair k taking the words from w1(k) and
// w2(k)).  Both sums of a pair have Z = dx = x2 - x1, a difference of two parked inputs, so the prefix products need no addition:
// pass 1, k = 0 .. N - 1: dx_k from the two x alone, the product p_k of the dx before it parked at prod0 + 9 (k - 1) (p_0 = 1 is not
// parked), p <- p dx_k -- one product a trip, the next trip's x2 requested before it; pass 2, k = N - 1 .. 0: the pair is added ONCE
// (5M + 3S), in registers, taken times p_k and the product of the dx behind it -- every pair on Z = prod dx -- and handed to out(k, r).
// s: prod dx.  P1 stays in registers over the trips that share it (w1 changes once or twice a batch).  AHEAD (S2K_R3_AHEAD, default 1):
// pass 2 also requests the next trip's x2, y2 and p_k before this trip's arithmetic -- 27 more live registers, which the kernel's 256
// VGPRs hold without scratch; 0 leaves the loads at the head of their own trip (for A/B builds).
struct ring3_pair { fe xp, yp, xm, ym, m, dx; };
S2K_HD void ring3_pair_add(ring3_pair& r, const fe& x1, const fe& y1, const fe& x2, const fe& y2) {
    fe dy, sy, t, c, d, d2, w1, w2, e, a1;
    fe_neg(t, x1, 1); fe_add2(r.dx, x2, t); fe_norm_weak(r.dx);
    fe_neg(t, y1, 1); fe_add2(dy, y2, t); fe_norm_weak(dy);
    fe_add2(sy, y1, y2); fe_norm_weak(sy);
    fe_sqr2(c, r.dx, d, dy);
    fe_mul2(w1, x1, c, w2, x2, c);
    fe_neg(e, w1, 1); fe_add(e, w2);                                  // dx^3                        (3)
    fe_mul_sqr(a1, y1, e, d2, sy);                                    // (1*3)
    fe_add2(t, w1, w2); fe_neg(t, t, 2);                              // -(W1 + W2)                  (3)
    fe_add2(r.xp, d, t); fe_add2(r.xm, d2, t);                        // X(P1 + P2), X(P1 - P2)      (4)
    fe_neg(t, r.xp, 4); fe_add(t, w1);                                // W1 - X3                     (6)
    fe_neg(e, w1, 1); fe_add(e, r.xm);                                // X3' - W1                    (6)
    fe_mul2(r.yp, dy, t, r.ym, sy, e);                                // (1*6, 1*6)
    fe_neg(t, a1, 1); fe_add(r.yp, t); fe_add(r.ym, t);               // Y = dy (W1 - X3) - y1 dx^3 ; Y' = sy (X3' - W1) - y1 dx^3   (3)
}
// pair r (m = product of the dx before it) times s (product of the dx behind it); s takes the pair's own dx in
S2K_HD void ring3_pair_scale(ring3_pair& r, fe& s) {
    fe m;
    fe_mul2(m, r.m, s, s, s, r.dx);
    fe m2, m3; fe_sqr(m2, m); fe_mul(m3, m2, m);
    fe_mul2(r.xp, r.xp, m2, r.xm, r.xm, m2);                          // (4*1)
    fe_mul2(r.yp, r.yp, m3, r.ym, r.ym, m3);                          // (3*1)
}
// ring3_pair_batch_xy: x2 of pair k at w2x(k) and y2 at w2y(k), which need not follow each other (the six-base form's P2 is a lambda
// image: beta x parked once per point, y shared with the point itself); ring3_pair_batch: the 18-word form, y2 at w2(k) + 9.
template <int N, int AHEAD, class W1, class W2X, class W2Y, class Out>
S2K_HD void ring3_pair_batch_xy(fe& s, u32* raw, int prod0, W1 w1, W2X w2, W2Y w2y, Out out) {
    {
        fe p, x1, x2, nx; fe_set_int(p, 1);
        rraw_load(x1, raw, w1(0)); rraw_load(x2, raw, w2(0));
#pragma unroll 1
        for (int k = 0; k < N; k++) {
            if (k + 1 < N) rraw_load(nx, raw, w2(k + 1));               // the next trip's x2, ahead of this trip's product
            if (k > 0 && w1(k) != w1(k - 1)) rraw_load(x1, raw, w1(k));
            fe dx, t;
            fe_neg(t, x1, 1); fe_add2(dx, x2, t); fe_norm_weak(dx);
            if (k > 0) rraw_store(raw, prod0 + 9 * (k - 1), p);
            fe_mul(p, p, dx);
            x2 = nx;
        }
    }
    fe_set_int(s, 1);
    ring3_pair r;
    fe x1, y1, x2, y2, nx, ny, nm;
    if (AHEAD) { rraw_load(x2, raw, w2(N - 1)); rraw_load(y2, raw, w2y(N - 1)); rraw_load(r.m, raw, prod0 + 9 * (N - 2)); }
#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
#pragma unroll
        for (int i = 0; i < 9; i++) S2K_OPAQUE(s.n[i]);                 // (carried around the 16-trip loop as it is, the compiler keeps s in register pairs and spends 390 more instructions a trip on s * dx)
        if (k == N - 1 || w1(k) != w1(k + 1)) { rraw_load(x1, raw, w1(k)); rraw_load(y1, raw, w1(k) + 9); }
        if (AHEAD) {
            if (k > 0) { rraw_load(nx, raw, w2(k - 1)); rraw_load(ny, raw, w2y(k - 1)); }
            if (k > 1) rraw_load(nm, raw, prod0 + 9 * (k - 2)); else fe_set_int(nm, 1);
        } else {
            rraw_load(x2, raw, w2(k)); rraw_load(y2, raw, w2y(k));
            if (k > 0) rraw_load(r.m, raw, prod0 + 9 * (k - 1)); else fe_set_int(r.m, 1);
        }
        ring3_pair_add(r, x1, y1, x2, y2);
        ring3_pair_scale(r, s);
        out(k, r);
        if (AHEAD) { x2 = nx; y2 = ny; r.m = nm; }
    }
}
template <int N, int AHEAD, class W1, class W2, class Out>
S2K_HD void ring3_pair_batch(fe& s, u32* raw, int prod0, W1 w1, W2 w2, Out out) {
    static_assert(N >= 2, "pass 2 requests the prefix product of pair N - 1 at prod0 + 9 (N - 2)");
    ring3_pair_batch_xy<N, AHEAD>(s, raw, prod0, w1, w2, [w2](int k) { return w2(k) + 9; }, out);
}
// C, T1 = 2^43*C, T2 = 2^86*C finite, magnitudes <= (5,3,1).  rtab: this lane's S2K_RTAB_WORDS; raw: this lane's column of its wavefront's
// parking area
S2K_HD void ecmult_ring3_tables(u32* rtab, u32* raw, const gej& C, const gej& T1, const gej& T2) {
    {   // the chains, all on the Z  za * z1 * z2  (which waits in the Z factor's place)
        fe za, z1, z2, zoa, zo1, zo2, zs;
        ptab_build_raw_n<2, S2K_RAW_WS, S2K_RAW_ES>(za, raw + S2K_R3_CHAIN0 * S2K_RAW_WS, C);
        ptab_build_raw_n<2, S2K_RAW_WS, S2K_RAW_ES>(z1, raw + (S2K_R3_CHAIN0 + 54) * S2K_RAW_WS, T1);
        ptab_build_raw_n<2, S2K_RAW_WS, S2K_RAW_ES>(z2, raw + (S2K_R3_CHAIN0 + 108) * S2K_RAW_WS, T2);
        fe_mul2(zoa, z1, z2, zo1, za, z2);                          // each chain by the product of the OTHER two's Z
        fe_mul(zo2, za, z1);
#pragma unroll 1
        for (int e = 5; e >= 0; e--) {
            if (e == 5) zs = zo2; else if (e == 3) zs = zo1; else if (e == 1) zs = zoa;
            const int src = S2K_R3_CHAIN0 + 27 * e, dst = e < 2 ? 18 * e : S2K_R3_T0 + 18 * (e - 2);
            fe x, y, h, zs2, zs3;
            rraw_load(x, raw, src); rraw_load(y, raw, src + 9); rraw_load(h, raw, src + 18);
            fe_sqr(zs2, zs); fe_mul(zs3, zs2, zs);
            fe_mul2(x, x, zs2, y, y, zs3);
            rraw_store(raw, dst, x); rraw_store(raw, dst + 9, y);
            fe_mul(zs, zs, h);                                      // ratio z_1 / z_0 joins the factor for the entry below
        }
        fe_mul(zs, zoa, za);
#pragma unroll
        for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = zs.n[i];
    }
    fe d1, d2;
    // stage 1: pair k = 2 (b - 1)/2 + (c - 1)/2 : b*T1 +- c*T2  ->  Q_2k = b*T1 + c*T2, Q_2k+1 = b*T1 - c*T2
    ring3_pair_batch<4, S2K_R3_AHEAD>(d1, raw, S2K_R3_S1PROD0,
        [](int k) { return S2K_R3_T0 + 18 * (k >> 1); }, [](int k) { return S2K_R3_T0 + 36 + 18 * (k & 1); },
        [&](int k, const ring3_pair& r) {
            const int q = S2K_R3_Q0 + 36 * k;
            rraw_store(raw, q, r.xp); rraw_store(raw, q + 9, r.yp); rraw_store(raw, q + 18, r.xm); rraw_store(raw, q + 27, r.ym);
        });
    {   // C, 3C onto D1
        fe m2, m3; fe_sqr(m2, d1); fe_mul(m3, m2, d1);
#pragma unroll 1
        for (int e = 0; e < 2; e++) {
            fe x, y; rraw_load(x, raw, 18 * e); rraw_load(y, raw, 18 * e + 9);
            fe_mul2(x, x, m2, y, y, m3);
            rraw_store(raw, 18 * e, x); rraw_store(raw, 18 * e + 9, y);
        }
    }
    // stage 2: pair k = 8 (a - 1)/2 + q : a*C +- Q_q, normalised and packed, two sectors the pair
    ring3_pair_batch<16, S2K_R3_AHEAD>(d2, raw, S2K_R3_PROD0,
        [](int k) { return 18 * (k >> 3); }, [](int k) { return S2K_R3_Q0 + 18 * (k & 7); },
        [&](int k, ring3_pair& r) {
            const int ai = k >> 3, bi = 2 + ((k >> 2) & 1), ca = (k >> 1) & 1, ci = (k & 1) ? 1 - ca : 2 + ca;      // (b + 3) / 2, (c + 3) / 2
            fe_normalize(r.xp); fe_normalize(r.yp); fe_normalize(r.xm); fe_normalize(r.ym);
            u32* const ep = rtab + (ai * 16 + bi * 4 + ci) * 16;                  // J(a, b, c)
            u32* const em = rtab + (ai * 16 + (3 - bi) * 4 + (3 - ci)) * 16;      // J(a, -b, -c)
            u32 wx[8], wy[8];
            fe_to_words(wx, r.xp); fe_to_words(wy, r.yp);
#pragma unroll
            for (int i = 0; i < 8; i++) { ep[i] = wx[i]; ep[8 + i] = wy[i]; }
            fe_to_words(wx, r.xm); fe_to_words(wy, r.ym);
#pragma unroll
            for (int i = 0; i < 8; i++) { em[i] = wx[i]; em[8 + i] = wy[i]; }
        });
    fe ziso;
#pragma unroll
    for (int i = 0; i < 9; i++) ziso.n[i] = rtab[S2K_RTAB_ZISO + i];
    fe_mul(d1, d1, d2); fe_mul(ziso, ziso, d1);                               // (a dx of zero makes the Z factor zero: the step then returns 0)
#pragma unroll
    for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = ziso.n[i];
}
// ---- the six-base form of the ring table (S2K_RING_SIX, rangeproof.h) ------------------------------------------------------------
// The same six pieces (sc_split_pieces3), but the lambda images of the three bases are bases of the table themselves: lambda*P is
// (beta x, y) on the same Z, so they cost nothing to put IN, and one operand then carries one signed bit of every piece of BOTH GLV
// halves.  A piece magnitude v is odd and below 2^43, so it is exactly 43 digits +-1: sum d_i 2^i = 2B - (2^43 - 1) with d_i = 2 b_i - 1,
// i.e. b is read off B = (v - 1)/2 + 2^42 -- bit t of B is bit t + 1 of v, bit 42 is set -- and there is no fixed top digit.  Level i has
// six signed digits (dC, d1, d2 of half 0; dC', d1', d2' of half 1) and takes
//     dC * E(dC d1, dC d2, dC dC', dC d1', dC d2') ,   E(u, v, w0, w1, w2) = C + u*T1 + v*T2 + w0*lambda C + w1*lambda T1 + w2*lambda T2 ,
// at sector (u < 0) + 2 (v < 0) + 4 (w0 < 0) + 8 (w1 < 0) + 16 (w2 < 0): again 32 sectors and the six-bit field neg << 5 | sector, field
// `level` (0 = most significant) five per word, 43 fields in the same nine digit words.
// A step is 43 levels of 1 doubling (none in front of the first) + 1 addition: 42 doublings, 43 operands the first of which is taken as
// it is, and no beta product.
// Construction (ecmult_ring6_tables): C and T1 brought to one Z (za z1 z2) in registers; the pair C +- T1 (Z = its dx, both sums parked);
// T2, parked as it came meanwhile, onto that Z in one go (by za z1 dx); the two pairs (C +- T1) +- T2 brought to the product of their two dx, which gives the four
//     A_a = C + u*T1 + v*T2 ,  a = (u < 0) + 2 (v < 0) ,
// and beta x of each; then the sixteen conjugate pairs A_i +- lambda A_j (pair k = 4 i + j; P2 = (beta x_j, y_j)):
// A_i + lambda A_j = E at sector i + 8 j, A_i - lambda A_j at that sector with bits 2..4 complemented; brought to the product of their
// sixteen dx by prefix / suffix products and packed (ring3_pair_batch_xy).  The Z factor is za z1 z2 times all nineteen dx.  No dx can
// vanish for a finite C (n would divide a small nonzero combination of 1, 2^43, 2^86 and their lambda multiples); one that does is a
// factor of the Z factor all the same, and a step that finds the Z factor zero returns 0.
// A lane's words of the parking area (word w at raw[w * S2K_RAW_WS]) during the construction -- W = 243 of the 32 x 27 are used, 324 are
// written per ring (18 + 36 + 18 + 9 + 72 + 36 + 135):
//     words   0..71   A_0..A_3, 18 words (x, y) each
//     words  72..107  beta x of A_0..A_3, 9 words each
//     words 108..242  the product of the dx before pair k, k = 1..15, 9 words each at 108 + 9 (k - 1) (that of pair 0 is 1)
//     before the sixteen pairs the same words hold: 108..143 C + T1, C - T1 (18 words each), 144..161 T2 (as it came, then on their Z), 162..170 the dx of
//     (C + T1) +- T2 (the one prefix product of that batch)
//     words 243..863  unused by this form
#define S2K_R6_LEVELS 43
#define S2K_R6_BX0 72
#define S2K_R6_PROD0 108
#define S2K_R6_P0 108
#define S2K_R6_T2 144
#define S2K_R6_S1PROD0 162
#define S2K_R6_PARK_WORDS 243                                   /* W: the highest used word + 1 */
// bit b_i (digit d_i = 2 b_i - 1, i = 0 least significant) of an odd piece magnitude below 2^43
S2K_HD u32 ring6_piece_bit(u64 m, int i) { return (u32)((((m >> 1) | (1ull << 42)) >> i) & 1ull); }
// the digit words 0..8 of a step: field `level`, level 0 = most significant, five six-bit fields per word
S2K_HD void ring6_recode(u32 dw[9], const piece43 pc[6]) {
#pragma unroll
    for (int i = 0; i < 9; i++) dw[i] = 0;
#pragma unroll
    for (int pos = 0; pos < S2K_R6_LEVELS; pos++) {
        const int i = S2K_R6_LEVELS - 1 - pos;
        u32 sg[6];
#pragma unroll
        for (int t = 0; t < 6; t++) sg[t] = (ring6_piece_bit(pc[t].m, i) ^ 1u) ^ (u32)pc[t].neg;
        const u32 v = sg[0] << 5 | (sg[2] ^ sg[0]) | (sg[4] ^ sg[0]) << 1 | (sg[1] ^ sg[0]) << 2 | (sg[3] ^ sg[0]) << 3 | (sg[5] ^ sg[0]) << 4;
        dw[pos / 5] |= v << ((pos % 5) * 6);
    }
}
// C, T1 = 2^43*C, T2 = 2^86*C finite, magnitudes <= (5,3,1).  rtab: this lane's S2K_RTAB_WORDS; raw: this lane's column of its wavefront's
// parking area
S2K_HD void ecmult_ring6_tables(u32* rtab, u32* raw, const gej& C, const gej& T1, const gej& T2) {
    {   // C and T1 onto the Z  za * z1 * z2 , their pair, T2 onto the pair's Z; the Z so far waits in the Z factor's place
        fe zoa, zo1, zo2, zs, x1, y1, x2, y2;
        x2 = T2.x; y2 = T2.y; fe_norm_weak(x2); fe_norm_weak(y2);
        rraw_store(raw, S2K_R6_T2, x2); rraw_store(raw, S2K_R6_T2 + 9, y2);     // (as it came, so that it is not live over the pair)
        fe_mul2(zoa, T1.z, T2.z, zo1, C.z, T2.z);                   // each base by the product of the OTHER two's Z
        fe_mul(zo2, C.z, T1.z);
        {
            fe m2, m3;
            x1 = C.x; y1 = C.y; fe_norm_weak(x1); fe_norm_weak(y1);
            fe_sqr(m2, zoa); fe_mul(m3, m2, zoa); fe_mul2(x1, x1, m2, y1, y1, m3);
            x2 = T1.x; y2 = T1.y; fe_norm_weak(x2); fe_norm_weak(y2);
            fe_sqr(m2, zo1); fe_mul(m3, m2, zo1); fe_mul2(x2, x2, m2, y2, y2, m3);
        }
        fe_mul(zs, zoa, C.z);
        ring3_pair r;
        ring3_pair_add(r, x1, y1, x2, y2);
        fe_norm_weak(r.xp); fe_norm_weak(r.yp); fe_norm_weak(r.xm); fe_norm_weak(r.ym);
        rraw_store(raw, S2K_R6_P0, r.xp); rraw_store(raw, S2K_R6_P0 + 9, r.yp); rraw_store(raw, S2K_R6_P0 + 18, r.xm); rraw_store(raw, S2K_R6_P0 + 27, r.ym);
        fe_mul2(zs, zs, r.dx, zo2, zo2, r.dx);
#pragma unroll
        for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = zs.n[i];
        {
            fe m2, m3;
            rraw_load(x2, raw, S2K_R6_T2); rraw_load(y2, raw, S2K_R6_T2 + 9);
            fe_sqr(m2, zo2); fe_mul(m3, m2, zo2); fe_mul2(x2, x2, m2, y2, y2, m3);
            rraw_store(raw, S2K_R6_T2, x2); rraw_store(raw, S2K_R6_T2 + 9, y2);
        }
    }
    fe d1, d2;
    // pair k: (C + T1) +- T2 (k = 0), (C - T1) +- T2 (k = 1)  ->  A_k (the sum), A_k+2 (the difference), and beta x of both
    ring3_pair_batch<2, S2K_R3_AHEAD>(d1, raw, S2K_R6_S1PROD0,
        [](int k) { return S2K_R6_P0 + 18 * k; }, [](int) { return S2K_R6_T2; },
        [&](int k, const ring3_pair& r) {
            fe beta, bp, bm; fe_set_beta(beta);
            fe_mul2(bp, r.xp, beta, bm, r.xm, beta);
            rraw_store(raw, 18 * k, r.xp); rraw_store(raw, 18 * k + 9, r.yp); rraw_store(raw, 18 * (k + 2), r.xm); rraw_store(raw, 18 * (k + 2) + 9, r.ym);
            rraw_store(raw, S2K_R6_BX0 + 9 * k, bp); rraw_store(raw, S2K_R6_BX0 + 9 * (k + 2), bm);
        });
    // pair k = 4 i + j : A_i +- lambda A_j, normalised and packed, two sectors the pair
    ring3_pair_batch_xy<16, S2K_R3_AHEAD>(d2, raw, S2K_R6_PROD0,
        [](int k) { return 18 * (k >> 2); }, [](int k) { return S2K_R6_BX0 + 9 * (k & 3); }, [](int k) { return 18 * (k & 3) + 9; },
        [&](int k, ring3_pair& r) {
            const int sp = (k >> 2) | ((k & 3) << 3);
            fe_normalize(r.xp); fe_normalize(r.yp); fe_normalize(r.xm); fe_normalize(r.ym);
            u32* const ep = rtab + sp * 16;                                       // A_i + lambda A_j
            u32* const em = rtab + (sp ^ 28) * 16;                                // A_i - lambda A_j
            u32 wx[8], wy[8];
            fe_to_words(wx, r.xp); fe_to_words(wy, r.yp);
#pragma unroll
            for (int i = 0; i < 8; i++) { ep[i] = wx[i]; ep[8 + i] = wy[i]; }
            fe_to_words(wx, r.xm); fe_to_words(wy, r.ym);
#pragma unroll
            for (int i = 0; i < 8; i++) { em[i] = wx[i]; em[8 + i] = wy[i]; }
        });
    fe ziso;
#pragma unroll
    for (int i = 0; i < 9; i++) ziso.n[i] = rtab[S2K_RTAB_ZISO + i];
    fe_mul(d1, d1, d2); fe_mul(ziso, ziso, d1);                               // (a dx of zero makes the Z factor zero: the step then returns 0)
#pragma unroll
    for (int i = 0; i < 9; i++) rtab[S2K_RTAB_ZISO + i] = ziso.n[i];
}
// e != 0; has_f uniform over the wavefront.  htab: this lane's generator's table (same layout as gtab).
// the digit words 0..8 of a step of the two-base forms from the GLV halves (joint form: ring_joint_recode; separate form: 5-bit digits
// (pos * 4 + stream), six per word, and the streams' signs in sneg)
S2K_HD void ring_step_recode(u32 dw[9], u32& sneg, const half_scalar& h0, const half_scalar& h1) {
    piece65 pc[4]; sc_split_pieces(pc, h0, h1);
#if S2K_RING_JOINT
    ring_joint_recode(dw, pc);
#else
#pragma unroll
    for (int i = 0; i < 9; i++) dw[i] = 0;
#pragma unroll
    for (int st = 0; st < 4; st++) {
        sneg |= (u32)pc[st].neg << st;
#pragma unroll
        for (int pos = 0; pos < S2K_RING_DIGITS; pos++) {            // pos 0 = most significant digit
            const int i = S2K_RING_DIGITS - 1 - pos, bit = S2K_RING_W * i + 1, word = bit >> 5, sh = bit & 31;
            const u64 pair = (u64)pc[st].w[word] | ((u64)(word + 1 < 3 ? pc[st].w[word + 1] : 0u) << 32);
            u32 v = (u32)(pair >> sh) & 31u;
            if (pos == 0) v |= 16u;                                  // bit 64 of B (the piece is below 2^65: bits 65, 66 are clear)
            const int nib = pos * 4 + st;
            dw[nib / 6] |= v << ((nib % 6) * 5);
        }
    }
#endif
}
// FORM = 1: the three-base form (above): 2 doublings a level and its own recoding; the fields sit where the joint form's do.
// FORM = 2: the six-base form: 1 doubling a level, one operand a level (field `level`), no lambda operand.  Its accumulator carries the signs
//           its next operation wants (group.h: gej_dblneg_ring, gej_rsub_ge_ring, gez_add_ge_ring): a level is R <- -2R, R <- operand - R with
//           -X handed back to the doubling; the table part runs on (-X, -Y, ZZ, ZZZ), which is where the hand-over leaves it once Z has
//           changed sign with Y ((X, Y, Z) and (X, -Y, -Z) are one point).
//           FRAC: R comes back as the fractions x = R.x / R.z, y = R.y / R.z (R.z = ZZ * ZZZ up to sign; a zero ZZ makes it zero), three
//           products from the XYZZ accumulator, for a caller that inverts R.z and takes two more (rangeproof.h); otherwise as Jacobian.
template <int FORM, bool FRAC = false>
S2K_HD int ecmult_ring_step_t(gej& R, const u32* rtab, const scalar& e, const scalar& s, const scalar& f, int has_f, const u32* gtab, const u32* htab,
                              const s2k_lds_ptr dig) {
    constexpr bool TRIPLE = FORM == 1, SIX = FORM == 2;
    constexpr int RING_W = TRIPLE ? 2 : S2K_RING_W, RING_GROUP = TRIPLE ? 2 : S2K_RING_GROUP;
    constexpr int RING_ADDS_P = SIX ? S2K_R6_LEVELS : TRIPLE ? 2 * S2K_R3_DIGITS : S2K_RING_ADDS_P;
    constexpr bool FIELDS = FORM || S2K_RING_JOINT;           // six-bit fields neg << 5 | sector in the digit words
    u32 sneg = 0; (void)sneg;                                   // (separate form only)
    S2K_PROF_DECL;
    {
        half_scalar h0, h1; sc_split_lambda_odd(h0, h1, e);
        u32 dw[9];
        if constexpr (SIX) { piece43 pc3[6]; sc_split_pieces3(pc3, h0, h1); ring6_recode(dw, pc3); }
        else if constexpr (TRIPLE) { piece43 pc3[6]; sc_split_pieces3(pc3, h0, h1); ring3_recode(dw, pc3); }
        else ring_step_recode(dw, sneg, h0, h1);
#pragma unroll
        for (int i = 0; i < 9; i++) dig[i * S2K_DIG_STRIDE] = dw[i];
        u32 sr[S2K_GTAB_SWORDS], fr[S2K_GTAB_SWORDS]; gtab_recode(sr, s.d, gtab); gtab_recode(fr, f.d, has_f ? htab : gtab);
#pragma unroll
        for (int i = 0; i < S2K_GTAB_SWORDS; i++) { dig[(9 + i) * S2K_DIG_STRIDE] = sr[i]; dig[(18 + i) * S2K_DIG_STRIDE] = fr[i]; }
    }
    S2K_PROF_MARK(1);
    const gtab_geom GG = gtab_geometry(gtab), GH = gtab_geometry(has_f ? htab : gtab);      // (the generator's table may have another width than G's)
    const int a_g0 = RING_ADDS_P, a_h0 = a_g0 + (int)GG.W;
    const int a_end = has_f ? a_h0 + (int)GH.W : a_h0;
    auto op_locate = [&](const u32*& addr, int& valid, int& neg, int idx) {
        addr = rtab; valid = 0; neg = 0;
        if (idx < a_g0) {
            if constexpr (FIELDS) {
                const u32 v = (dig[(idx / 5) * S2K_DIG_STRIDE] >> ((idx % 5) * 6)) & 63u;   // ring_joint_field / ring3_field / ring6_recode
                valid = 1;
                neg = (int)(v >> 5);
                addr = rtab + (v & 31u) * 16;
            } else {
                const int st = idx & 3;
                const u32 v = (dig[(idx / 6) * S2K_DIG_STRIDE] >> ((idx % 6) * 5)) & 31u;
                valid = 1;
                neg = (v < 16u) ^ (int)((sneg >> st) & 1u);
                const u32 en = (v < 16u) ? (15u - v) : (v - 16u);
                addr = rtab + (st >> 1) * S2K_RTAB_TABLE_WORDS + en * 16;
            }
        } else if (idx < a_end) {
            const int second = idx >= a_h0;
            const int g = idx - (second ? a_h0 : a_g0), base = second ? 18 : 9, w = (int)(((u32)g * (second ? GH.D : GG.D)) >> 5);
            valid = gtab_locate(addr, neg, second ? htab : gtab, second ? GH : GG, g, dig[(base + w) * S2K_DIG_STRIDE], w + 1 < S2K_GTAB_SWORDS ? dig[(base + 1 + w) * S2K_DIG_STRIDE] : 0u);
        }
    };
    auto op_decode = [&](ge& o, const u32 raw[16], int neg, int lam) {
        fe y, yn;
        fe_from_words(o.x, raw); fe_from_words(y, raw + 8);
        if (lam) { fe beta; fe_set_beta(beta); fe_mul(o.x, o.x, beta); }          // `lam` is a compile-time constant at every call site
        fe_neg(yn, y, 1);
        fe_select(o.y, yn, y, neg);
    };
    const u32* nxt_addr; int nxt_valid, nxt_neg;
    u32 raw[16];
    ge cur; int cur_valid;
    op_locate(nxt_addr, nxt_valid, nxt_neg, 0);
#pragma unroll
    for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
    op_decode(cur, raw, nxt_neg, 0);
    op_locate(nxt_addr, nxt_valid, nxt_neg, 1);
    // variable part, separate form: additions 0..51 as 26 (plain stream, lambda stream) pairs, 5 doublings in front of every group of four
    // but the first; joint form: additions 0..43 as 22 such pairs, one per level, 3 doublings in front of every pair but the first (three-base
    // form: 2 doublings); six-base form: additions 0..42, one per level, 1 doubling in front of every one but the first
    int au = 0;
    if constexpr (SIX) {
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
        gej_set_ge(R, cur); fe_neg(R.x, R.x, 1);                            // level 0: the operand as it is, X carried as -X (2)
        au = 1;
        op_decode(cur, raw, nxt_neg, 0); cur_valid = nxt_valid;
        op_locate(nxt_addr, nxt_valid, nxt_neg, 2);
#pragma unroll 1
        while (au < a_g0) {
            S2K_PROF_MARK(7);
            gej_dblneg_ring<true>(R, R);
            S2K_PROF_MARK(6);
#pragma unroll
            for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];              // request the next record before the arithmetic
            { const int same_x = gej_rsub_ge_ring(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
            au++;
            op_decode(cur, raw, nxt_neg, 0); cur_valid = nxt_valid;
            op_locate(nxt_addr, nxt_valid, nxt_neg, au + 1);
        }
    } else
    while (au < a_g0) {
        if (au >= RING_GROUP && !(au & (RING_GROUP - 1))) {
            S2K_PROF_MARK(7);
#pragma unroll 1
            for (int k = 0; k < RING_W; k++) gej_double_lean(R, R);
            S2K_PROF_MARK(6);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];                  // request the next record before the arithmetic
        if (au == 0) gej_set_ge(R, cur);
        else { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        op_decode(cur, raw, nxt_neg, 1);                                    // operand of the lambda stream
        op_locate(nxt_addr, nxt_valid, nxt_neg, au + 2);
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
        { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        au += 2;
        op_decode(cur, raw, nxt_neg, 0); cur_valid = nxt_valid;
        op_locate(nxt_addr, nxt_valid, nxt_neg, au + 1);
    }
    S2K_PROF_MARK(7);
    {   // back to the real curve
        fe zi;
#pragma unroll
        for (int i = 0; i < 9; i++) zi.n[i] = rtab[S2K_RTAB_ZISO + i];
        fe_mul(R.z, R.z, zi);
        // a Z factor of zero (joint form: a table whose construction met a dx of zero) makes ZZ zero below, it stays zero through the table
        // part, and the one ZZ test behind it sends the step back; only the form without that test needs one of its own
#if !S2K_XYZZ_TABLE_PART
        if (FIELDS && S2K_WAVE_ANY(fe_normalizes_to_zero(zi))) return 0;
#endif
    }
    // table part (G, then H): a zero window adds nothing (per lane), so these additions are committed by select
#if S2K_XYZZ_TABLE_PART
    gez acc4; acc4.inf = 0; acc4.x = R.x; acc4.y = R.y;
    if constexpr (SIX) {                                                    // R = (-X, Y, Z) = (-X, -(-Y), -(-Z)): over -Z both coordinates are carried negated
        fe nz; fe_neg(nz, R.z, 1);                                          // (2: squared as it is, 1*2 in the product)
        fe_sqr(acc4.zz, nz); fe_mul(acc4.zzz, acc4.zz, nz);
    } else {
        fe_sqr(acc4.zz, R.z); fe_mul(acc4.zzz, acc4.zz, R.z);
    }
#else
    if constexpr (SIX) { fe_neg(R.x, R.x, 1); fe_norm_weak(R.x); }
#endif
    while (au < a_end) {
#if S2K_NT_GTAB && defined(__HIP_DEVICE_COMPILE__)
        {
            typedef unsigned int s2k_u32x4 __attribute__((ext_vector_type(4)));
            const s2k_u32x4* q = (const s2k_u32x4*)nxt_addr;
#pragma unroll
            for (int k = 0; k < 4; k++) { const s2k_u32x4 v = __builtin_nontemporal_load(q + k); raw[4 * k] = v.x; raw[4 * k + 1] = v.y; raw[4 * k + 2] = v.z; raw[4 * k + 3] = v.w; }
        }
#else
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
#endif
#if S2K_XYZZ_TABLE_PART
        {
            gez t = acc4;
            if constexpr (SIX) gez_add_ge_ring(t, cur); else gez_add_ge_lean(t, cur);
            if (S2K_WAVE_ALL(cur_valid)) acc4 = t;               // (a zero digit -- one window value in 2^D -- is the only reason for the selects)
            else { fe_cmov(acc4.x, t.x, cur_valid); fe_cmov(acc4.y, t.y, cur_valid); fe_cmov(acc4.zz, t.zz, cur_valid); fe_cmov(acc4.zzz, t.zzz, cur_valid); }
        }
#else
        gej t; const int same_x = gej_add_ge_lean(t, R, cur);
        if (S2K_WAVE_ANY(same_x & cur_valid)) return 0;
        if (cur_valid) R = t;
#endif
        au++;
        op_decode(cur, raw, nxt_neg, 0); cur_valid = nxt_valid;
        op_locate(nxt_addr, nxt_valid, nxt_neg, au + 1);
    }
#if S2K_XYZZ_TABLE_PART
    if (S2K_WAVE_ANY(fe_normalizes_to_zero(acc4.zz))) return 0;      // some committed addition met an operand with the accumulator's own x
    if constexpr (SIX) {
        R.inf = 0;
        if constexpr (FRAC) {                                           // x = X / ZZ = (-X) ZZZ / (-ZZ ZZZ), y = Y / ZZZ = (-Y) ZZ / (-ZZ ZZZ)
            fe nzz; fe_neg(nzz, acc4.zz, 1);                            // (2)
            fe_mul2(R.x, acc4.x, acc4.zzz, R.y, acc4.y, acc4.zz);       // (2*1, 1*1)
            fe_mul(R.z, nzz, acc4.zzz);
        } else {                                                        // (-X ZZ, -Y ZZZ, ZZ) with the two signs put right
            fe_mul2(R.x, acc4.x, acc4.zz, R.y, acc4.y, acc4.zzz);
            fe_neg(R.x, R.x, 1); fe_neg(R.y, R.y, 1); fe_norm_weak(R.x); fe_norm_weak(R.y);
            R.z = acc4.zz;
        }
    } else gej_set_gez(R, acc4);
#endif
    S2K_PROF_MARK(10);
#ifdef S2K_ON_RING_STEP_DONE
    S2K_ON_RING_STEP_DONE();
#endif
    return 1;
}
S2K_HD int ecmult_ring_step(gej& R, const u32* rtab, const scalar& e, const scalar& s, const scalar& f, int has_f, const u32* gtab, const u32* htab,
                            const s2k_lds_ptr dig) {
    return ecmult_ring_step_t<0>(R, rtab, e, s, f, has_f, gtab, htab, dig);
}
S2K_HD int ecmult_ring3_step(gej& R, const u32* rtab, const scalar& e, const scalar& s, const scalar& f, int has_f, const u32* gtab, const u32* htab,
                             const s2k_lds_ptr dig) {
    return ecmult_ring_step_t<1>(R, rtab, e, s, f, has_f, gtab, htab, dig);
}
S2K_HD int ecmult_ring6_step(gej& R, const u32* rtab, const scalar& e, const scalar& s, const scalar& f, int has_f, const u32* gtab, const u32* htab,
                             const s2k_lds_ptr dig) {
    return ecmult_ring_step_t<2>(R, rtab, e, s, f, has_f, gtab, htab, dig);
}
// the same with R as the fractions over R.z (FRAC above; with the table part that is not on XYZZ there is nothing to take them from)
#define S2K_RING6_FRAC (S2K_XYZZ_TABLE_PART != 0)
S2K_HD int ecmult_ring6_step_frac(gej& R, const u32* rtab, const scalar& e, const scalar& s, const scalar& f, int has_f, const u32* gtab, const u32* htab,
                                  const s2k_lds_ptr dig) {
    return ecmult_ring_step_t<2, S2K_RING6_FRAC>(R, rtab, e, s, f, has_f, gtab, htab, dig);
}


// ---- the joint form: two variable points, no generator  R = na*A + nb*B ----------------------------------------------------------------
// (the DLEQ half of an adaptor signature needs s*Y - e*R, adaptor.h; the reference takes two secp256k1_ecmult calls and a gej_add_var for it,
// src/modules/ecdsa_adaptor/dleq_impl.h:146-150: 256 doublings and 132 table additions.)  Both points get a table of odd multiples, the two
// tables are rescaled to ONE common Z exactly as in ecmult_lane_split (the second table slot of the lane's slice), and the GLV halves of na
// (on A) and of nb (on B) run as four digit streams of 33 signed odd 4-bit digits, the top one fixed: 128 doublings and 132 additions, the
// first of which just takes its operand.  Digit stream in LDS: words 0..15 = nibble (pos * 4 + stream), streams 0, 1 = the halves of na,
// 2, 3 = those of nb.  Only the lock-step form exists: the function returns 0 without having produced anything when the wavefront is not
// uniform (a lane with A.inf, B.inf or a zero scalar), when a lane meets an operand with the accumulator's own x coordinate, or when the
// two tables cannot share a Z (a Z of zero: only points off the curve get there); the caller then runs ecmult_lane2_calls below.
#define S2K_JOINT_ADDS (4 * 33)
S2K_HD int ecmult_lane2(gej& R, const gej& A, const scalar& na, const gej& B, const scalar& nb, const lane_mem& lm) {
    u32* const ptab = lm.ptab; const s2k_lds_ptr dig = lm.dig;
    const int active = (!A.inf) & (!B.inf) & (!sc_is_zero(na)) & (!sc_is_zero(nb));
    if (!S2K_WAVE_ALL(active)) return 0;
    u32 sneg = 0;                                                    // bit st: stream st is negative
    S2K_PROF_DECL;
    {
        u32 dw[16];
#pragma unroll
        for (int i = 0; i < 16; i++) dw[i] = 0;
        auto put = [&](const half_scalar& h, const int st) {             // the 32 digits of one stream into their nibbles (st a constant)
            sneg |= (u32)h.neg << st;
#pragma unroll
            for (int pos = 0; pos < 32; pos++) {                         // pos 0 = digit 31 (most significant after the fixed top digit)
                const int i = 31 - pos, bit = 4 * i + 1, word = bit >> 5, sh = bit & 31;
                const u64 pair = (u64)h.w[word] | ((u64)h.w[word + 1] << 32);      // (word <= 3)
                const u32 v = (u32)(pair >> sh) & 15u;
                const int nib = pos * 4 + st;
                dw[nib >> 3] |= v << ((nib & 7) * 4);
            }
        };
        { half_scalar h0, h1; sc_split_lambda_odd(h0, h1, na); put(h0, 0); put(h1, 1); }
        { half_scalar h0, h1; sc_split_lambda_odd(h0, h1, nb); put(h0, 2); put(h1, 3); }
#pragma unroll
        for (int i = 0; i < 16; i++) dig[i * S2K_DIG_STRIDE] = dw[i];
        fe za, zb, ziso;
        S2K_PROF_MARK(1);
        ptab_build_raw(za, ptab, A);
        ptab_build_raw(zb, ptab + S2K_PTAB_TABLE_WORDS, B);
        fe_mul(ziso, za, zb);
        if (S2K_WAVE_ANY(fe_normalizes_to_zero(ziso))) return 0;
        S2K_PROF_MARK(8);
        ptab_rescale(ptab, &zb);
        ptab_rescale(ptab + S2K_PTAB_TABLE_WORDS, &za);
        S2K_PROF_MARK(9);
#pragma unroll
        for (int i = 0; i < 9; i++) ptab[S2K_PTAB_ZISO + i] = ziso.n[i];
    }
    auto op_locate = [&](const u32*& addr, int& neg, int idx) {
        const int st = idx & 3;
        u32 v = 8u;                                                                     // the fixed top digit +1
        if (idx >= 4 && idx < S2K_JOINT_ADDS) { const int nib = idx - 4; v = (dig[(nib >> 3) * S2K_DIG_STRIDE] >> ((nib & 7) * 4)) & 15u; }
        neg = (v < 8u) ^ (int)((sneg >> st) & 1u);
        const u32 e = (v < 8u) ? (7u - v) : (v - 8u);
        addr = ptab + (st >> 1) * S2K_PTAB_TABLE_WORDS + e * S2K_PTAB_ENTRY_WORDS + (((st & 1) && S2K_PTAB_TWINS) ? 16 : 0);
    };
    auto op_decode = [&](ge& o, const u32 raw[16], int neg, int lam) {
        fe y, yn;
        fe_from_words(o.x, raw); fe_from_words(y, raw + 8);
        if (lam) { fe beta; fe_set_beta(beta); fe_mul(o.x, o.x, beta); }          // `lam` is a compile-time constant at every call site
        fe_neg(yn, y, 1);
        fe_select(o.y, yn, y, neg);
    };
    const u32* nxt_addr; int nxt_neg;
    u32 raw[16];
    ge cur;
    op_locate(nxt_addr, nxt_neg, 0);
#pragma unroll
    for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
    op_decode(cur, raw, nxt_neg, 0);
    op_locate(nxt_addr, nxt_neg, 1);
    // additions 0..131 as 66 (plain stream, lambda stream) pairs, as in ecmult_lane_split; 4 doublings in front of every group of four
    // but the first.  In place: a lane that meets its own x coordinate makes the caller start over.  (Past the last addition op_locate
    // wraps to the fixed top digit: a request for a record of the lane's own table that nobody decodes.)
    int au = 0;
    while (au < S2K_JOINT_ADDS) {
        if (au >= 4 && !(au & 3)) {
#pragma unroll 1
            for (int k = 0; k < 4; k++) gej_double_lean(R, R);
            S2K_PROF_MARK(6);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];                  // request the next record before the arithmetic
        if (au == 0) gej_set_ge(R, cur);
        else { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        op_decode(cur, raw, nxt_neg, !S2K_PTAB_TWINS);                      // operand of the lambda stream
        op_locate(nxt_addr, nxt_neg, au + 2);
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = nxt_addr[k];
        { const int same_x = gej_add_ge_lean(R, R, cur); if (S2K_WAVE_ANY(same_x)) return 0; }
        au += 2;
        op_decode(cur, raw, nxt_neg, 0);
        op_locate(nxt_addr, nxt_neg, au + 1);
    }
    { fe zi; ptab_load_ziso(zi, ptab); fe_mul(R.z, R.z, zi); }             // back to the real curve
    S2K_PROF_MARK(10);
#ifdef S2K_ON_JOINT_DONE
    S2K_ON_JOINT_DONE();                                                                      // host test build: count completed joint runs
#endif
    return 1;
}

// A Jacobian point parked in memory between two multiplications, so that it is not held in registers across one: 28 words, `stride`
// words apart (the kernels interleave the lanes of a launch: word k of every lane side by side).
#define S2K_PARK_GEJ_WORDS 28
S2K_HD void gej_park(u32* p, size_t stride, const gej& a) {
    fe x = a.x, y = a.y, z = a.z;
    fe_norm_weak(x); fe_norm_weak(y); fe_norm_weak(z);
#pragma unroll
    for (int i = 0; i < 9; i++) { p[i * stride] = x.n[i]; p[(9 + i) * stride] = y.n[i]; p[(18 + i) * stride] = z.n[i]; }
    p[27 * stride] = (u32)a.inf;
}
S2K_HD void gej_unpark(gej& a, const u32* p, size_t stride) {
#pragma unroll
    for (int i = 0; i < 9; i++) { a.x.n[i] = p[i * stride]; a.y.n[i] = p[(9 + i) * stride]; a.z.n[i] = p[(18 + i) * stride]; }
    a.inf = (int)p[27 * stride];
}
// The same sum as the reference takes it: two ecmult_lane calls and a gej_add_var (every input is served: infinity, zero scalars, A = +-B).
// The first product waits in `park` (S2K_PARK_GEJ_WORDS words of this lane) while the second is computed.
// load(k, P, n) hands in term k (0: A and na, 1: B and nb) when it is needed, so that a kernel can read its inputs again from global
// memory instead of holding the second term in registers across the first multiplication.
template <class Load>
S2K_HD void ecmult_lane2_calls(gej& R, Load load, const u32* gtab, const lane_mem& lm, u32* park, size_t park_stride) {
    scalar zero; sc_set_zero(zero);
    {
        gej P, T; scalar n;
        load(0, P, n);
        ecmult_lane(T, P, n, zero, 0, gtab, lm);
        gej_park(park, park_stride, T);
    }
    gej P, T, F; scalar n;
    load(1, P, n);
    ecmult_lane(T, P, n, zero, 0, gtab, lm);
    gej_unpark(F, park, park_stride);
    gej_add_var(R, F, T);
}
// An offset of zero the compiler cannot see through: inputs read again through it are loaded again, not kept from the first time.
S2K_HD u32 s2k_opaque_zero() { u32 z = 0; S2K_CHAIN(z); return z; }
