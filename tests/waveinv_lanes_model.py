"""Python model of the lane-distributed uniform inverse (csrc/modinv.h: ds_inverse_words_lanes), vectorised over many inputs with numpy.

One row of 16 "lanes" (a DPP row) per input: lane i (0..8) holds limb i of f, g, d, e, lanes 9..15 hold zeros.  Every machine operation
is modelled at its width: 32-bit words wrap by explicit masks, every 64-bit sum is checked for leaving the signed 64-bit range, every
value that the device keeps in a 32-bit register is checked to fit one, and the limb ranges that the header comment of the device code
states are asserted after every batch.  `exact_batches` is the same computation on Python integers, without limbs.

Shared by tests/test_cpu_wave_inverse_lanes.py (which guards the bounds) and tests/test_gpu_wave_inverse_lanes.py."""
import numpy as np

BITS, LIMBS, BATCHES, LANES = 30, 9, 20, 16
MASK = (1 << BITS) - 1
M32 = (1 << 32) - 1
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
# the device's modulus constants (DS_MOD_P: a sparse signed form; DS_MOD_N: canonical limbs) and m^-1 mod 2^30
MODS = {
    "p": (P, [-977, -4, 0, 0, 0, 0, 0, 0, 65536], 0x2DDACACF),
    "n": (N, [(N >> (BITS * i)) & MASK for i in range(LIMBS)], 0x2A774EC1),
}
# stated bounds (modinv.h): limbs 0..7 between batches, the column sums
LIMB_LO, LIMB_HI = -3, (1 << BITS) + 2
SUM_MAX = (1 << BITS) * ((1 << BITS) + 3) + (1 << BITS) * ((1 << BITS) - 1)
I32_LO, I32_HI = -(1 << 31), (1 << 31) - 1


def limbs_of(v):
    return [(v >> (BITS * i)) & MASK for i in range(LIMBS)]


def value_of(limbs):
    return sum(int(x) << (BITS * i) for i, x in enumerate(limbs[:LIMBS]))


def _fits32(x):
    return bool(((x >= I32_LO) & (x <= I32_HI)).all())


def _add64(x, y):
    """x + y on int64 arrays; the sum must not leave the signed 64-bit range"""
    s = x + y                                   # numpy wraps
    assert not (((x ^ s) & (y ^ s)) < 0).any(), "64-bit sum out of range"
    return s


def _ctz32(x):
    x = x | (1 << 31)
    return np.log2((x & -x).astype(np.float64)).astype(np.int64)


def batch(zeta, f, g):
    """ds_batch / ds_batch_uniform: 30 division steps on the low words (int64 arrays holding 32-bit words).  -> zeta, (u, v, q, r)"""
    n = len(f)
    u, v, q, r = np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64)
    left = np.full(n, BITS, np.int64)
    zeta, f, g = zeta.copy(), f.copy(), g.copy()
    while (left > 0).any():
        z = np.minimum(_ctz32(g), left)
        g >>= z; u <<= z; v <<= z; zeta -= z; left -= z
        act = left > 0
        sw = act & (zeta < 0)
        fm = np.where(sw, (-f) & M32, f)
        um, vm = np.where(sw, -u, u), np.where(sw, -v, v)
        g2 = ((g + fm) & M32) >> 1
        q2, r2 = q + um, r + vm
        f = np.where(sw, g, f); u = np.where(sw, q, u); v = np.where(sw, r, v)
        g = np.where(act, g2, g); q = np.where(act, q2, q); r = np.where(act, r2, r)
        zeta = np.where(sw, -zeta - 2, zeta - act)
        u <<= act; v <<= act; left -= act
    for a, b in ((u, v), (q, r)):
        assert (np.abs(a) + np.abs(b) <= (1 << BITS)).all()
    return zeta, (u, v, q, r)


_LANE = np.arange(LANES)
_LM = np.where(_LANE < LIMBS - 1, MASK, -1).astype(np.int64)
_CM = np.where(_LANE < LIMBS - 1, -1, 0).astype(np.int64)


def _from_above(x):                             # row_shl:1: lane i <- lane i + 1, 0 into the row's last lane
    return np.concatenate([x[:, 1:], np.zeros((len(x), 1), np.int64)], axis=1)


def _from_below(x):                             # row_shr:1: lane i <- lane i - 1, 0 into lane 0
    return np.concatenate([np.zeros((len(x), 1), np.int64), x[:, :-1]], axis=1)


def _carry(s):
    """dsl_carry: column sums (int64) -> limbs (int32)"""
    lo = s & MASK
    mid_full = s >> BITS
    assert _fits32(mid_full[:, LIMBS - 1:]), "top lane's S >> 30 does not fit 32 bits"
    mid = np.where(_LANE < LIMBS - 1, mid_full & MASK, mid_full)
    top = s >> (2 * BITS)
    u = _from_above(lo) + mid
    assert _fits32(u)
    c = ((u >> BITS) + top) & _CM
    r = (u & _LM) + _from_below(c)
    assert _fits32(r)
    return r


def _mul(t, a):
    """(int64) t * a, both 32-bit operands of v_mad_i64_i32"""
    assert _fits32(t) and _fits32(a)
    return t[:, None] * a


def carry(s):
    """dsl_carry on rows of 16 column sums (lanes 9..15 zero), every register width asserted"""
    return _carry(np.asarray(s, dtype=np.int64))


class Run:
    """results: the inverses; batches: how many batches the device runs (early exit included); states[it] = (f, g, d, e) limb arrays
    (n, 16) after batch it; sum_max / sum_min: the largest and smallest column sum of each input over all batches, lanes and numbers"""


def run(values, mod, record=False, stop=BATCHES):
    m, mlimbs, inv = MODS[mod]
    n = len(values)
    mrow = np.zeros(LANES, np.int64); mrow[:LIMBS] = mlimbs
    f = np.tile(mrow, (n, 1))
    g = np.zeros((n, LANES), np.int64)
    g[:, :LIMBS] = np.array([limbs_of(v) for v in values], dtype=np.int64).reshape(n, LIMBS)
    d = np.zeros((n, LANES), np.int64)
    e = np.zeros((n, LANES), np.int64); e[:, 0] = 1
    zeta = np.full(n, -1, np.int64)
    out = Run()
    out.batches = np.full(n, BATCHES, np.int64)
    out.states = []
    out.sum_max = np.full(n, -(1 << 62), np.int64)
    out.sum_min = np.full(n, 1 << 62, np.int64)
    done = np.zeros(n, bool)
    final_f, final_d = f.copy(), d.copy()
    for it in range(min(stop, BATCHES)):
        zeta, (t00, t01, t10, t11) = batch(zeta, f[:, 0] & M32, g[:, 0] & M32)
        d0, e0 = (d[:, 0] & M32).astype(np.uint64), (e[:, 0] & M32).astype(np.uint64)
        w = lambda x: (x & M32).astype(np.uint64)
        inv64, m32 = np.uint64(inv), np.uint64(M32)
        with np.errstate(over="ignore"):
            ka = ((np.uint64(0) - (((w(t00) * d0 + w(t01) * e0) & m32) * inv64)) & np.uint64(MASK)).astype(np.int64)
            kb = ((np.uint64(0) - (((w(t10) * d0 + w(t11) * e0) & m32) * inv64)) & np.uint64(MASK)).astype(np.int64)
        mm = np.tile(mrow, (n, 1))
        sd = _add64(_add64(_mul(t00, d), _mul(t01, e)), _mul(ka, mm))
        se = _add64(_add64(_mul(t10, d), _mul(t11, e)), _mul(kb, mm))
        sf = _add64(_mul(t00, f), _mul(t01, g))
        sg = _add64(_mul(t10, f), _mul(t11, g))
        for s in (sd, se, sf, sg):
            assert (np.abs(s) <= SUM_MAX).all(), "column sum beyond the stated bound"
            assert ((s[:, 0] & MASK) == 0).all()
            live = ~done
            out.sum_max[live] = np.maximum(out.sum_max[live], s[live].max(axis=1))
            out.sum_min[live] = np.minimum(out.sum_min[live], s[live].min(axis=1))
        d, e, f, g = _carry(sd), _carry(se), _carry(sf), _carry(sg)
        for a in (d, e, f, g):
            assert ((a[:, :LIMBS - 1] >= LIMB_LO) & (a[:, :LIMBS - 1] <= LIMB_HI)).all(), "limb beyond the stated bound"
            assert ((a[:, 0] >= 0) & (a[:, 0] <= MASK)).all(), "lane 0 is not exact"
            assert (np.abs(a[:, LIMBS - 1]) < (1 << 22)).all(), "top limb beyond 2^22"
            assert (a[:, LIMBS:] == 0).all(), "a lane above 8 is not zero"
        if record:
            out.states.append((f.copy(), g.copy(), d.copy(), e.copy()))
        live = ~done
        final_f[live], final_d[live] = f[live], d[live]
        if it >= BATCHES - 5:
            z = g.copy()                         # the exit test: g's carries rippled all the way, on a copy
            for _ in range(LIMBS - 1):
                z = (z & _LM) + _from_below((z >> BITS) & _CM)
                assert _fits32(z)
            assert ((z[:, :LIMBS - 1] >= 0) & (z[:, :LIMBS - 1] <= MASK)).all()
            ex = live & (z == 0).all(axis=1)
            out.batches[ex] = it + 1
            done |= ex
    out.results = []
    if stop < BATCHES:
        return out
    for i, v in enumerate(values):
        fv, dv = value_of(final_f[i]), value_of(final_d[i])
        assert abs(dv) < 21 * m
        if v % m == 0:
            assert abs(fv) == m and dv % m == 0
        else:
            assert abs(fv) == 1
        out.results.append((dv if fv > 0 else -dv) % m)
    return out


def exact_batches(v, mod, stop=BATCHES):
    """the same batches on Python integers: [(f, g, d, e)] after every batch, and the first batch count at which g is 0 (None if never)"""
    m, _, inv = MODS[mod]
    f, g, d, e, zeta = m, v, 0, 1, np.full(1, -1, np.int64)
    states, g_zero_at = [], None
    for it in range(stop):
        zeta, t = batch(zeta, np.array([f & M32], np.int64), np.array([g & M32], np.int64))
        t00, t01, t10, t11 = (int(x[0]) for x in t)
        ka = (-(t00 * d + t01 * e) * inv) & MASK
        kb = (-(t10 * d + t11 * e) * inv) & MASK
        nd, ne = t00 * d + t01 * e + ka * m, t10 * d + t11 * e + kb * m
        nf, ng = t00 * f + t01 * g, t10 * f + t11 * g
        assert nd & MASK == 0 and ne & MASK == 0 and nf & MASK == 0 and ng & MASK == 0
        d, e, f, g = nd >> BITS, ne >> BITS, nf >> BITS, ng >> BITS
        states.append((f, g, d, e))
        if g == 0 and g_zero_at is None:
            g_zero_at = it + 1
    return states, g_zero_at
