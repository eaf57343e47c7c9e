"""CPU tier: what a generator-cache slot keeps for the rangeproof prologue (csrc/rangeproof.h on the host, tests/host_emul/rp_cached_bases_emu.cpp).

* the slot's ring-base chain (rp_gen_chain, one call per exponent index) holds word for word the records rp_pp_bases writes per proof:
  bases[i] = record i, dbases[i] = record 32 + i, for every exponent index, for full and short proofs, with and without dbases;
* the records are the points they claim to be: record i = -(4^i 10^exp) * gen (checked in affine form with plain integers);
* the slot's is-square flag equals Euler's criterion on the generator's y, and rp_pp_hash computes the same message hash when it is
  handed the flag as when it takes the square root itself -- for H (y not a square), -H (a square) and two more, and the wrong flag
  changes it."""
import ctypes
import json
import os

import numpy as np
import pytest

from secp256k1_zkp_amd.constants import GENERATOR_H, P

HERE = os.path.dirname(os.path.abspath(__file__))


def _neg(gen64):
    return gen64[:32] + ((P - int.from_bytes(gen64[32:], "big")) % P).to_bytes(32, "big")


def _lift(x):
    """some curve point with the x coordinate `x` or the next one that has a point (p = 3 mod 4)"""
    while True:
        y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
        if y * y % P == (x * x * x + 7) % P:
            return x.to_bytes(32, "big") + y.to_bytes(32, "big")
        x += 1


GENS = [GENERATOR_H, _neg(GENERATOR_H), _lift(0x1234567890ABCDEF << 128), _neg(_lift(7))]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_rp_cached_bases_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_rp_cached_bases_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    for f in (lib.emu_rp_chain_recs, lib.emu_rp_chain_exps, lib.emu_rp_gej_words):
        f.restype = ctypes.c_uint
    lib.emu_rp_gen_chain.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lib.emu_rp_pp_bases.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_int]
    lib.emu_rp_gen_y_is_square.argtypes = [ctypes.c_char_p]
    lib.emu_rp_hash.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def chains(emu):
    """gen -> [exps][recs][words], built once"""
    E, R, W = emu.emu_rp_chain_exps(), emu.emu_rp_chain_recs(), emu.emu_rp_gej_words()
    assert (E, R, W) == (19, 64, 28)
    out = {}
    for g in GENS:
        c = np.zeros((E, R, W), np.uint32)
        for e in range(E):
            emu.emu_rp_gen_chain(c[e].ctypes.data, g, e)
        out[g] = c
    return out


def _pp_bases(emu, g, rings, exp, with_d=True):
    b = np.full((32, 28), 0xDEADBEEF, np.uint32); d = np.full((32, 28), 0xDEADBEEF, np.uint32)
    emu.emu_rp_pp_bases(b.ctypes.data, d.ctypes.data if with_d else None, g, rings, exp)
    return b, d


@pytest.mark.parametrize("gi", range(len(GENS)))
def test_chain_equals_rp_pp_bases_word_for_word(emu, chains, gi):
    g = GENS[gi]; c = chains[g]
    for exp in range(-1, 19):
        e_idx = max(exp, 0)
        for rings in (32, 1, 2, 31) if exp in (-1, 0, 7, 18) else (32,):
            b, d = _pp_bases(emu, g, rings, exp)
            assert np.array_equal(b[:rings], c[e_idx, :rings]), (exp, rings)
            assert np.array_equal(d[:rings], c[e_idx, 32:32 + rings]), (exp, rings)
            assert (b[rings:] == 0xDEADBEEF).all() and (d[rings:] == 0xDEADBEEF).all()          # rp_pp_bases writes the proof's rings only
    b, d = _pp_bases(emu, g, 5, 3, with_d=False)                                                     # (no dbases: the chain stops at the last ring)
    assert np.array_equal(b[:5], c[3, :5]) and (d == 0xDEADBEEF).all()


def _fe(words):
    return sum(int(w) << (29 * i) for i, w in enumerate(words)) % P          # csrc/fe.h: 9 limbs of 29 bits, lazily reduced


def _affine(rec):
    x, y, z = _fe(rec[0:9]), _fe(rec[9:18]), _fe(rec[18:27])
    assert rec[27] == 0 and z != 0
    zi = pow(z, -1, P)
    return x * zi * zi % P, y * zi * zi * zi % P


def _add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def _mul(k, pt):
    r = None
    while k:
        if k & 1:
            r = _add(r, pt)
        pt = _add(pt, pt); k >>= 1
    return r


def test_chain_records_are_the_ring_bases(chains):
    g = GENS[2]; c = chains[g]
    neg = (int.from_bytes(g[:32], "big"), P - int.from_bytes(g[32:], "big"))
    for e in (0, 1, 18):
        pt = _mul(10**e, neg)
        for i in range(64):
            assert _affine(c[e, i]) == pt, (e, i)
            pt = _add(pt, pt); pt = _add(pt, pt)


def test_is_square_flag_and_message_hash(emu):
    fx = json.load(open(os.path.join(HERE, "golden", "rangeproof_exceptional.json")))
    commit, proof = bytes.fromhex(fx["commit33"]), bytes.fromhex(fx["proof"])
    flags = []
    for g in GENS:
        y = int.from_bytes(g[32:], "big")
        sq = int(pow(y, (P - 1) // 2, P) == 1)
        assert emu.emu_rp_gen_y_is_square(g) == sq
        flags.append(sq)
        m = [np.zeros(8, np.uint32) for _ in range(3)]
        for k, gsq in enumerate((-1, sq, 1 - sq)):
            assert emu.emu_rp_hash(m[k].ctypes.data, commit, proof, len(proof), g, gsq) == 1
        assert np.array_equal(m[0], m[1]) and not np.array_equal(m[0], m[2])
    assert flags[:2] == [0, 1]                                   # exactly one of y and -y is a square (p = 3 mod 4): for H it is -y
