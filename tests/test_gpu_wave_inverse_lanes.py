"""The lane-distributed uniform inverse (csrc/modinv.h: ds_inverse_words_lanes) on the device, for both moduli, one value per wavefront:
against Python's pow, against the scalar-apply form (ds_inverse_words<true>) bit for bit, and -- batch by batch -- against the Python
model of the lane scheme (tests/waveinv_lanes_model.py), limb for limb.  Workgroups of 64 and of 256 lanes."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import waveinv_lanes_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
DUMP_WORDS = 4 * M.LIMBS * M.BATCHES
MODSEL = {"p": 0, "n": 1}

# Seeds (random.Random(SLOW_SEED_BASE[mod] + seed).randrange(1, m)) of the values that needed the most batches among 4 000 seeded values
# per modulus under the model: 18 for every one of them (3 788 of 4 000 for p, 3 776 for n; the others 17), and 18 is also where the
# model on Python integers (exact_batches) says their g reaches 0.  No seeded value needed 19 or 20.
SLOW_SEED_BASE = {"p": 1000003, "n": 2000006}
SLOW_SEEDS = {"p": [0, 1, 2, 3, 4, 5], "n": [0, 1, 2, 3, 4, 5]}
SLOW_BATCHES = 18

# Carry edges: inputs whose first two batches give the largest and smallest column sums found.
#  * constructed: limb 0 = m mod 2^30 makes the first batch's matrix (0, 2^30; -1, 1) (one swap, then 29 even steps), so f <- g and the
#    lanes with a limb of 2^30 - 1 form S = 2^30 (2^30 - 1) = 2^60 - 2^30, the most canonical limbs can give an (f, g) sum;
#  * found by a search over 30 000 values of limb 0 under limbs of 2^30 - 1: for n a (d, e) sum of 2^60 + 8.67e15 in batch 2, for p a sum
#    of -(2^59 + 4.0e9), the smallest seen.
# The stated maximum, 2^61 + 2^31, needs limbs at their redundant extremes under a row of (2^30, 0) or (0, 2^30) and k m at its own
# extreme with the same sign all at once; no input within 2^20 of it, or of its negative, was found or constructed: these are 2^60 away.
CARRY_EDGES = {
    "p": [M.value_of([M.P & M.MASK, M.MASK - 5, M.MASK, M.MASK, M.MASK, M.MASK, M.MASK, M.MASK, 0xFFFF]),
          0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffebffffc2f,
          0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffea3de0507],
    "n": [M.value_of([M.N & M.MASK, M.MASK, M.MASK, M.MASK, 0x3FFFFEB0, M.MASK, M.MASK, M.MASK, 0xFFFF]),
          0xfffffffffffffffffffffffffffffffeb0fffffffffffffffffffffff6433f95,
          0xfffffffffffffffffffffffffffffffeb0ffffffffffffffffffffffcda42d70],
}
CARRY_EDGE_SUMS = {"p": (1152921503533105152, -576460754316689408), "n": (1161594351386935389, -7615841646411776)}


def edge_values(m):
    return [1, 2, m - 1, m - 2, (m + 1) // 2, (1 << 255) % m, 1 << 30, (1 << 30) - 1, 1 << 240, 0]


@pytest.fixture(scope="module")
def uinv(engine):
    import torch
    lib = ctypes.CDLL(os.path.join(HERE, "wave_inverse", "libs2k_waveinv_lanes_test.so"))

    def run(form, mod, values, block=64):
        """one wavefront per value.  -> results (one per value; all 64 lanes must agree), and for form 2 the state dump and batch counts"""
        nw = len(values)
        words = np.array([[(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for v in values], dtype=np.uint32)
        tin = torch.tensor(words.view(np.int32).reshape(-1)).cuda()
        out = torch.full((nw * 64 * 8,), -1, dtype=torch.int32, device="cuda")
        dump = torch.zeros(nw * DUMP_WORDS, dtype=torch.int32, device="cuda")
        nb = torch.full((nw,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = lib.s2k_test_uniform_inverse(form, MODSEL[mod], ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(dump.data_ptr()),
                                          ctypes.c_void_p(nb.data_ptr()), ctypes.c_void_p(tin.data_ptr()), nw * 64, block)
        assert ok == 1
        w = out.cpu().numpy().view(np.uint32).reshape(nw, 64, 8)
        assert (w == w[:, :1, :]).all(), "the lanes of a wavefront disagree"
        res = [sum(int(w[i, 0, j]) << (32 * j) for j in range(8)) for i in range(nw)]
        return res, dump.cpu().numpy().reshape(nw, M.BATCHES, 4, M.LIMBS), nb.cpu().numpy()
    return run


def _check_values(uinv, mod, vals):
    m = M.MODS[mod][0]
    exp = [pow(v, -1, m) if v else 0 for v in vals]
    while len(vals) % 4:                             # whole workgroups of 256
        vals, exp = vals + [vals[-1]], exp + [exp[-1]]
    for block in (64, 256):
        lanes, _, _ = uinv(0, mod, vals, block)
        scal, _, _ = uinv(1, mod, vals, block)
        assert scal == exp
        assert lanes == exp


def _check_states(uinv, mod, vals, block=64):
    """the device's limbs after every batch = the model's; their values = the batches on Python integers; d, e congruent and bounded"""
    m = M.MODS[mod][0]
    vals = list(vals)
    while len(vals) % 4:
        vals.append(vals[-1])
    model = M.run(vals, mod, record=True)
    res, dump, nb = uinv(2, mod, vals, block)
    assert res == model.results
    assert (nb == model.batches).all()
    for i, v in enumerate(vals):
        exact, _ = M.exact_batches(v, mod)
        for it in range(int(nb[i])):
            for k in range(4):                      # f, g, d, e: limb for limb
                assert (dump[i, it, k] == model.states[it][k][i, :M.LIMBS]).all(), (i, it, k)
            f, g, d, e = (M.value_of(dump[i, it, k]) for k in range(4))
            assert (f, g) == exact[it][:2], (i, it)
            assert (d - exact[it][2]) % m == 0 and (e - exact[it][3]) % m == 0, (i, it)
            assert abs(d) < 21 * m and abs(e) < 21 * m
            for k in range(4):
                assert dump[i, it, k, :M.LIMBS - 1].min() >= M.LIMB_LO and dump[i, it, k, :M.LIMBS - 1].max() <= M.LIMB_HI
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("mod", ["p", "n"])
def test_uniform_inverse_edge_values(uinv, mod):
    _check_values(uinv, mod, edge_values(M.MODS[mod][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("mod", ["p", "n"])
def test_uniform_inverse_random(uinv, mod):
    m = M.MODS[mod][0]
    rnd = random.Random(900 + ord(mod))
    _check_values(uinv, mod, [rnd.randrange(m) for _ in range(512)])


@pytest.mark.gpu
@pytest.mark.parametrize("mod", ["p", "n"])
def test_uniform_inverse_slowest_exits(uinv, mod):
    m = M.MODS[mod][0]
    vals = [random.Random(SLOW_SEED_BASE[mod] + s).randrange(1, m) for s in SLOW_SEEDS[mod]]
    for v in vals:
        assert M.exact_batches(v, mod)[1] == SLOW_BATCHES
    _check_values(uinv, mod, vals)
    model = _check_states(uinv, mod, vals)
    assert (model.batches == SLOW_BATCHES).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mod", ["p", "n"])
def test_uniform_inverse_state_after_every_batch(uinv, mod):
    m = M.MODS[mod][0]
    rnd = random.Random(77 + ord(mod))
    vals = [rnd.randrange(1, m) for _ in range(10)] + [1, m - 1, (m + 1) // 2, 1 << 30, 1 << 240, 0]
    _check_states(uinv, mod, vals)
    _check_states(uinv, mod, vals, block=256)


@pytest.mark.gpu
@pytest.mark.parametrize("mod", ["p", "n"])
def test_uniform_inverse_carry_edges(uinv, mod):
    """The largest and smallest column sums that could be constructed or found for the first two batches (CARRY_EDGES above): +2^60 - 2^30
    and +2^60 + 8.67e15 (n), -(2^59 + 4.0e9) (p).  The stated per-lane maximum is 2^61 + 2^31: these inputs stay 2^60 and more away from
    it and from its negative, not within 2^20; nothing nearer was found.  The carry step itself is taken to +-(2^61 + 2^31) and to every edge
    of its split on column sums handed in directly: test_lane_carry_at_the_stated_bound."""
    vals = CARRY_EDGES[mod]
    assert all(0 < v < M.MODS[mod][0] for v in vals)
    first = M.run(vals, mod, stop=2)
    assert int(first.sum_max[0]) == (1 << 60) - (1 << 30)
    assert (int(first.sum_max.max()), int(first.sum_min.min())) == CARRY_EDGE_SUMS[mod]
    _check_values(uinv, mod, vals)
    _check_states(uinv, mod, vals)


def carry_edge_rows():
    """Rows of column sums at and next to the stated bound +-SUM_MAX = +-(2^61 + 2^31), whether or not an inversion can produce them: every
    split S = top 2^60 + mid 2^30 + lo with top in [-3, 2], mid and lo in {0, 1, 2, 2^30 - 2, 2^30 - 1} that lies within the bound, the bound
    itself and its neighbours; lane 8 (the signed top limb: |S >> 30| < 2^22) with its own extremes.  First every extreme in all of lanes
    0..7 at once, then seeded mixtures, so that each meets each as its neighbour below and above, lane 7 next to lane 8 included."""
    small = [0, 1, 2, M.MASK - 1, M.MASK]
    ext = sorted({(top << 60) + (mid << 30) + lo for top in range(-3, 3) for mid in small for lo in small} |
                 {sg * (M.SUM_MAX - k) for sg in (1, -1) for k in (0, 1, 2, (1 << 20), (1 << 30) - 1, 1 << 30, (1 << 30) + 1)})
    ext = [x for x in ext if abs(x) <= M.SUM_MAX]
    top8 = [0, M.MASK, -1, (1 << 52) - 1, -(1 << 52) + 1, ((1 << 22) - 1) << 30, -(((1 << 22) - 1) << 30), ((1 << 21) << 30) + M.MASK, -(1 << 30), -(1 << 30) - 1]
    rows = [[x] * 8 + [t] + [0] * 7 for x in ext for t in (top8[0], top8[3], top8[4])]
    rnd = random.Random(4242)
    rows += [[rnd.choice(ext) for _ in range(8)] + [rnd.choice(top8)] + [0] * 7 for _ in range(4096 - len(rows) % 4096)]
    return np.array(rows, dtype=np.int64)


@pytest.mark.gpu
def test_lane_carry_at_the_stated_bound(engine):
    """dsl_carry on the device against the model's carry, limb for limb, on column sums at +-SUM_MAX and around every edge of its three-way
    split: top = -3 and +2, carries of -3 and +3, lo and mid all ones, in lanes 0..7 and under the signed lane 8.  The outputs must also
    lie in the limb range the header states, [-3, 2^30 + 2], and reach both of its ends."""
    import torch
    lib = ctypes.CDLL(os.path.join(HERE, "wave_inverse", "libs2k_waveinv_lanes_test.so"))
    rows = carry_edge_rows()
    assert int(rows.max()) == M.SUM_MAX and int(rows.min()) == -M.SUM_MAX
    tops = rows[:, :8] >> 60
    assert int(tops.min()) == -3 and int(tops.max()) == 2
    exp = M.carry(rows)
    assert int(exp[:, 1:8].min()) == M.LIMB_LO and int(exp[:, 1:8].max()) == M.LIMB_HI
    assert int(exp[:, :8].min()) >= M.LIMB_LO and int(exp[:, :8].max()) <= M.LIMB_HI and (exp[:, 9:] == 0).all()
    nw = len(rows)
    full = np.zeros((nw, 64), dtype=np.int64); full[:, :16] = rows
    for block in (64, 256):
        tin = torch.from_numpy(full.reshape(-1).copy()).cuda()
        out = torch.full((nw * 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert lib.s2k_test_lane_carry(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(tin.data_ptr()), nw * 64, block) == 1
        got = out.cpu().numpy().reshape(nw, 64)
        assert (got[:, :16] == exp).all()
        assert (got[:, 16:] == 0).all()
