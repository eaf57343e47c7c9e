"""CPU tier: the three-base form of the ring table (csrc/ecmult.h: one table indexed by the digits on C, 2^43 C and 2^86 C, 42 doublings a
step) on the host (tests/host_emul/ring_triple_emu.cpp, S2K_VERIFY on): the recoding on integers, every table entry and the step list of
tests/ring_joint_cases.py against the unmodified reference, and the layout's bounds under the address sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.refapi import G_XY, N
from tests.ring_joint_cases import b32, reference, split_bound_scalars, step_list
from tests.ring_triple_cases import HANDBACK_ALLOWED
from tests.test_cpu_ring_joint import _golden_small_x_points

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = ctypes.c_ulonglong


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_triple_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_triple_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_r3_piece_digits.argtypes = [ctypes.POINTER(ctypes.c_int), U64]
    return lib


@pytest.fixture(scope="module")
def steps(ref):
    C, e, s, f, kinds = step_list(ref)
    want, winf = reference(ref, C, e, s, f)
    assert not winf.any()
    return C, e, s, f, kinds, want


def test_sizes_stay_what_the_joint_form_pins(emu):
    out = (ctypes.c_int * 4)()
    emu.emu_r3_sizes(out)
    assert list(out) == [528, 2 * 16 * 27 * 64, 2 * 16 * 27, 27]


def _piece_values():
    rng = np.random.default_rng(9401)
    vals = [1, 3, 2**42 - 1, 2**42 + 1, 2**43 - 1, 2**44 - 1]
    vals += [int(rng.integers(0, 2**43, dtype=np.uint64)) * 2 + 1 for _ in range(200)]
    assert all(v & 1 and v < 2**44 for v in vals) and any(v > 2**43 for v in vals)
    return vals


def test_digits_resum_to_the_piece(emu):
    for v in _piece_values():
        d = (ctypes.c_int * 22)()
        emu.emu_r3_piece_digits(d, v)
        assert all(x in (-3, -1, 1, 3) for x in d)
        assert sum(x * 4**i for i, x in enumerate(d)) == v, hex(v)


def _pieces_of_halves(emu, halves):
    """halves: two signed odd integers below 2^129 in magnitude -> six signed pieces [C k1, C k2, T1 k1, T1 k2, T2 k1, T2 k2]"""
    hw = (ctypes.c_uint32 * 10)(*[(abs(h) >> (32 * i)) & 0xFFFFFFFF for h in halves for i in range(5)])
    hn = (ctypes.c_int * 2)(*[int(h < 0) for h in halves])
    m = (U64 * 6)(); neg = (ctypes.c_int * 6)()
    emu.emu_r3_pieces_of_halves(m, neg, hw, hn)
    return list(m), list(neg)


def _check_pieces(m, neg, halves):
    for hf in range(2):
        p = [(-m[2 * b + hf] if neg[2 * b + hf] else m[2 * b + hf]) for b in range(3)]
        assert p[0] + 2**43 * p[1] + 2**86 * p[2] == halves[hf], (hf, hex(halves[hf]))
        assert all(abs(x) & 1 and abs(x) <= 2**43 for x in p), (hf, hex(halves[hf]))


def test_pieces_of_the_halves_of_e(emu):
    """p0 + 2^43 p1 + 2^86 p2 with their signs is the signed half, every piece odd and at most 2^43: the split-bound scalars of the step
    list, random e, and halves given directly whose upper pieces are all even (both borrows taken) and all odd (none), at both signs"""
    rng = np.random.default_rng(9402)
    es = list(split_bound_scalars()) + [int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1 for _ in range(200)]
    for e in es:
        m = (U64 * 6)(); neg = (ctypes.c_int * 6)(); hw = (ctypes.c_uint32 * 10)(); hn = (ctypes.c_int * 2)()
        emu.emu_r3_pieces(m, neg, hw, hn, b32(e % N))
        halves = [(-1 if hn[hf] else 1) * sum(hw[5 * hf + i] << (32 * i) for i in range(5)) for hf in range(2)]
        assert all(h & 1 and abs(h) < 2**129 for h in halves)
        _check_pieces(list(m), list(neg), halves)
    mk = lambda p0, p1, p2: p0 + 2**43 * p1 + 2**86 * p2
    top = 2**43 - 1
    given = [mk(1, 0, 0), mk(1, 0, 2), mk(top, 0, top - 1), mk(1, 2, 4), mk(top, top - 1, top - 1),          # upper pieces all even
             mk(1, 1, 1), mk(top, top, top), mk(5, 3, 2**42 + 1), mk(top, top, 1),                            # upper pieces all odd
             mk(1, 0, 1), mk(1, 1, 0), mk(top, top, 0), mk(3, top - 1, top), 2**129 - 1, 2**128 + 1, 1]       # mixed, and the ends of the range
    for h in given:
        for s0, s1 in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            halves = [s0 * h, s1 * given[(given.index(h) + 3) % len(given)]]
            m, neg = _pieces_of_halves(emu, halves)
            _check_pieces(m, neg, halves)


def _decode(fld):
    sign = -1 if fld >> 5 else 1
    return sign * (2 * ((fld >> 4) & 1) + 1), sign * (2 * ((fld >> 2) & 3) - 3), sign * (2 * (fld & 3) - 3)


def test_field_selects_the_signed_triple(emu):
    """every (field on C, on T1, on T2) and sign pattern: neg << 5 | sector with sector = ((a - 1) / 2) * 16 + ((b + 3) / 2) * 4 + (c + 3) / 2
    selects +-J(a, b, c) whose three multipliers are the signed digits"""
    seen = set()
    for vc in range(4):
        for v1 in range(4):
            for v2 in range(4):
                for sg in range(8):
                    sc, s1, s2 = sg & 1, (sg >> 1) & 1, sg >> 2
                    want = tuple((2 * v - 3) * (-1 if s else 1) for v, s in ((vc, sc), (v1, s1), (v2, s2)))
                    fld = emu.emu_r3_field(vc, v1, v2, sc, s1, s2)
                    assert 0 <= fld < 64 and _decode(fld) == want, (vc, v1, v2, sg)
                    seen.add(fld)
    assert len(seen) == 64


def _fields(dw):
    return [(dw[idx // 5] >> ((idx % 5) * 6)) & 63 for idx in range(44)]


def test_recode_words_hold_the_fields_of_the_six_pieces(emu):
    """the nine digit words of a step: field (level * 2 + half), five to a word; summed back over the levels the selected multiples are the
    six signed pieces"""
    pcs = _piece_values()
    rng = np.random.default_rng(9403)
    for t in range(0, len(pcs) - 5, 3):
        p = pcs[t:t + 6]; neg = [int(x) for x in rng.integers(0, 2, 6)]
        if t < 24:
            neg = [(t // 3 >> i) & 1 for i in range(3)] * 2
            neg[3] ^= 1
        dw = (ctypes.c_uint32 * 9)()
        emu.emu_r3_recode(dw, (U64 * 6)(*p), (ctypes.c_int * 6)(*neg))
        tot = [0] * 6
        for idx, fld in enumerate(_fields(dw)):
            level, hf = idx >> 1, idx & 1
            for b, d in enumerate(_decode(fld)):
                tot[2 * b + hf] += d * 4**(21 - level)
        assert tot == [(-v if s else v) for v, s in zip(p, neg)]
        assert dw[8] >> 24 == 0                                  # 44 fields: the 45th place stays clear


def _table_points(ref):
    rng = np.random.default_rng(9404)
    g = np.frombuffer(G_XY, np.uint8)
    g2, _ = ref.ecmult_batch(g.reshape(1, 64), np.frombuffer(b32(2), np.uint8).reshape(1, 32))
    pts = [g, g2[0]] + [np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(8)]
    return pts + [np.frombuffer(c, np.uint8) for _, c in _golden_small_x_points()[:4]]


def test_every_table_entry(emu, ref):
    """all 32 sectors, taken back to the real curve with the Z factor, equal (a + b 2^43 + c 2^86) C: G, 2G, eight random points and the
    points with x below 2^32 that tests/golden holds"""
    ks = []
    for sector in range(32):
        a, b, c = _decode(sector)
        ks.append(np.frombuffer(b32((a + b * 2**43 + c * 2**86) % N), np.uint8))
    for c in _table_points(ref):
        out = ctypes.create_string_buffer(2048)
        assert emu.emu_r3_table(out, c.tobytes()) == 1
        want, winf = ref.ecmult_batch(np.tile(c, (32, 1)), np.stack(ks))
        assert not winf.any() and out.raw == want.tobytes()


def test_step_list(emu, steps):
    """every step equals the reference's (with the caller's fallback where it hands back); no random triple hands back, a listed multiplier
    only where tests/ring_triple_cases.py names it with its colliding sum (none is named: every listed multiplier completes)"""
    C, e, s, f, kinds, want = steps
    back = []
    for i in range(len(e)):
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        inf = emu.emu_r3_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 0)
        assert inf == 0 and out.raw == want[i].tobytes(), (i, kinds[i])
        if not took.value:
            back.append((kinds[i], int.from_bytes(e[i].tobytes(), "big")))
    assert not [k for k in back if k[0] != "listed"], back
    listed = sorted({v for _, v in back})
    assert len(HANDBACK_ALLOWED) <= 2 and set(listed) <= set(HANDBACK_ALLOWED), back


def test_zero_z_factor_hands_back(emu, steps):
    """a table whose Z factor is zero (what a dx of zero in the construction leaves) makes the step return 0; the fallback gives the result"""
    C, e, s, f, kinds, want = steps
    for i in [k for k, kind in enumerate(kinds) if kind == "random"][:4]:
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        assert emu.emu_r3_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 1) == 0
        assert took.value == 0 and out.raw == want[i].tobytes()


def test_layout_fits_under_the_address_sanitizer():
    """tests/host_emul/ring_triple_bounds (its own main, -fsanitize=address,undefined with the sanitizers' runtimes linked statically)
    builds a table and runs steps with rtab of exactly 528 and a parking area of exactly 864 words, both on the heap, as a child process
    in the environment the test itself runs in"""
    prog = os.path.join(HERE, "host_emul", "ring_triple_bounds")
    assert os.path.exists(prog), "tests/host_emul/ring_triple_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
