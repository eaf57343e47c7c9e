"""The wave-batched field inverse (csrc/waveinv.h: fe_inv_wave) on the device against the per-lane fe_inv and fe_inv_fermat and against
Python: random values, a wavefront of equal values, 1 and p - 1, lazily reduced inputs at the magnitude limit of fe_inv (2), and the
zero report (one lane = 0 mod p gives 0 on every lane of its wavefront, and only there)."""
import ctypes
import os

import numpy as np
import pytest

from tests.refapi import P

HERE = os.path.dirname(os.path.abspath(__file__))
LIMB_MAX = 2 * ((1 << 29) + (1 << 20))          # magnitude 2 (fe.h): limbs 0..7
TOP_MAX = 2 * ((1 << 24) + (1 << 10))           # and limb 8


@pytest.fixture(scope="module")
def waveinv(engine):
    import torch
    lib = ctypes.CDLL(os.path.join(HERE, "wave_inverse", "libs2k_waveinv_test.so"))

    def run(op, limbs, block=64):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint32)
        n = limbs.shape[0]
        tin = torch.tensor(limbs.view(np.int32).reshape(-1)).cuda()
        out = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        flag = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = lib.s2k_test_waveinv(op, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(flag.data_ptr()), ctypes.c_void_p(tin.data_ptr()), n, block)
        assert ok == 1
        w = out.cpu().numpy().view(np.uint32).reshape(n, 8)
        return [sum(int(w[i, j]) << (32 * j) for j in range(8)) for i in range(n)], flag.cpu().numpy()
    return run


def _limbs(v):
    """canonical 9 x 29-bit limbs of v < 2^256"""
    return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]


def _value(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def _check(waveinv, rows, block=64):
    rows = np.array(rows, dtype=np.uint64)
    vals = [_value(r) % P for r in rows]
    got, flag = waveinv(0, rows, block)
    lane, _ = waveinv(1, rows, block)
    ferm, _ = waveinv(2, rows, block)
    for w in range(len(vals) // 64):
        has_zero = any(v == 0 for v in vals[64 * w:64 * w + 64])
        assert (flag[64 * w:64 * w + 64] == (0 if has_zero else 1)).all(), w
    for i, v in enumerate(vals):
        exp = pow(v, -1, P) if v else 0
        assert lane[i] == exp and ferm[i] == exp, i
        if not flag[i]:
            continue
        assert got[i] == exp, i


@pytest.mark.gpu
def test_wave_inverse_random(waveinv):
    rng = np.random.default_rng(11)
    rows = [_limbs(int.from_bytes(rng.bytes(32), "little") % P) for _ in range(64 * 16)]
    _check(waveinv, rows)
    _check(waveinv, rows, block=256)             # four wavefronts per workgroup: the lane index is the one inside the wavefront


@pytest.mark.gpu
def test_wave_inverse_equal_lanes(waveinv):
    rng = np.random.default_rng(12)
    rows = []
    for _ in range(4):
        v = int.from_bytes(rng.bytes(32), "little") % P
        rows += [_limbs(v)] * 64
    _check(waveinv, rows)


@pytest.mark.gpu
def test_wave_inverse_one_and_minus_one(waveinv):
    rows = [_limbs(1)] * 64 + [_limbs(P - 1)] * 64 + [_limbs(1 if i % 2 else P - 1) for i in range(64)]
    _check(waveinv, rows)


@pytest.mark.gpu
def test_wave_inverse_magnitude_limits(waveinv):
    rng = np.random.default_rng(13)
    top = [LIMB_MAX] * 8 + [TOP_MAX]
    rows = [top] * 64                                                    # every limb at the limit
    rows += [[int(rng.integers(LIMB_MAX - (1 << 20), LIMB_MAX + 1)) for _ in range(8)] + [int(rng.integers(TOP_MAX - (1 << 10), TOP_MAX + 1))]
             for _ in range(64)]                                          # near it
    rows += [[int(rng.integers(0, LIMB_MAX + 1)) for _ in range(8)] + [int(rng.integers(0, TOP_MAX + 1))] for _ in range(128)]
    rows += [[a + b for a, b in zip(_limbs(int.from_bytes(rng.bytes(32), "little") % P), _limbs(P))] for _ in range(64)]     # x + p, limb-wise
    for r in rows:
        assert all(x <= LIMB_MAX for x in r[:8]) and r[8] <= TOP_MAX
    _check(waveinv, rows)


@pytest.mark.gpu
def test_wave_inverse_zero_report(waveinv):
    rng = np.random.default_rng(14)
    rows = [_limbs(int.from_bytes(rng.bytes(32), "little") % P) for _ in range(64 * 4)]
    rows[64 + 17] = [0] * 9                       # wavefront 1: a lane that is 0
    rows[128 + 63] = _limbs(P)                    # wavefront 2: a lane that is p (0 mod p, not normalised)
    rows[192 + 0] = [a + b for a, b in zip(_limbs(P), _limbs(P))]       # wavefront 3: 2p, lane 0
    _check(waveinv, rows)
    _, flag = waveinv(0, np.array(rows, dtype=np.uint64))
    assert flag[:64].all() and not flag[64:].any()
