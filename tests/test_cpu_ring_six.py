"""CPU tier: the six-base form of the ring table (csrc/ecmult.h: one table over C, 2^43 C, 2^86 C and their lambda images, one signed bit of
each per operand, 43 levels of one doubling and one addition) on the host (tests/host_emul/ring_six_emu.cpp, S2K_VERIFY on): the recoding
on integers, every table entry and the step list of tests/ring_triple_cases.py against the unmodified reference and the three-base form,
a dx of zero in each of the construction's three batches, and the parking map's bounds under the address sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.refapi import G_XY, N
from tests.ring_joint_cases import b32, reference, split_bound_scalars, step_list
from tests.ring_triple_cases import HANDBACK_ALLOWED
from tests.test_cpu_oracle import LAMBDA
from tests.test_cpu_ring_joint import _golden_small_x_points

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = ctypes.c_ulonglong
PARK_WORDS = 243                                      # W: highest used word + 1 of a lane's parking map (csrc/ecmult.h, above S2K_R6_LEVELS)
LEVELS = 43
# sector bit t belongs to the piece (index in sc_split_pieces3's order: C k1, C k2, T1 k1, T1 k2, T2 k1, T2 k2)
BIT_PIECE = (2, 4, 1, 3, 5)
# multiplier of each piece's base: 1, lambda, 2^43, lambda 2^43, 2^86, lambda 2^86
BASE_K = (1, LAMBDA, 2**43, LAMBDA * 2**43 % N, 2**86, LAMBDA * 2**86 % N)


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_six_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_six_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_r6_table_words.argtypes = [ctypes.c_void_p] + [ctypes.c_char_p] * 3 + [ctypes.c_int]
    lib.emu_r6_step_bases.argtypes = [ctypes.c_char_p] * 7 + [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def steps(ref):
    C, e, s, f, kinds = step_list(ref)
    want, winf = reference(ref, C, e, s, f)
    assert not winf.any()
    return C, e, s, f, kinds, want


def test_sizes_stay_what_the_other_forms_pin(emu):
    out = (ctypes.c_int * 6)()
    emu.emu_r6_sizes(out)
    assert list(out) == [528, 2 * 16 * 27 * 64, 2 * 16 * 27, 27, PARK_WORDS, 18]


def _digits(fld):
    """field neg << 5 | sector -> the six signed digits +-1 in the pieces' order"""
    d = [0] * 6
    d[0] = -1 if fld >> 5 else 1
    for t, piece in enumerate(BIT_PIECE):
        d[piece] = -d[0] if (fld >> t) & 1 else d[0]
    return d


def _resum(dw):
    """the nine digit words -> the six signed pieces that the 43 fields select, summed over the levels"""
    assert dw[8] >> 18 == 0                                   # 43 fields: the 44th and 45th places stay clear
    tot = [0] * 6
    for level in range(LEVELS):
        fld = (dw[level // 5] >> ((level % 5) * 6)) & 63
        for t, d in enumerate(_digits(fld)):
            tot[t] += d << (LEVELS - 1 - level)
    return tot


def _recode(emu, m, neg):
    dw = (ctypes.c_uint32 * 9)()
    emu.emu_r6_recode(dw, (U64 * 6)(*m), (ctypes.c_int * 6)(*neg))
    return list(dw)


def test_fields_cover_the_sign_patterns():
    assert len({tuple(_digits(f)) for f in range(64)}) == 64


def test_recode_gives_back_the_six_pieces(emu):
    """every odd magnitude below 2^43 is 43 digits +-1 with no fixed top digit: the ends 1 and 2^43 - 1, their neighbours, random ones; all
    64 sign patterns on the first values, random signs on the rest"""
    rng = np.random.default_rng(9701)
    vals = [1, 2**43 - 1, 3, 2**43 - 3, 2**42 - 1, 2**42 + 1] + [int(rng.integers(0, 2**42, dtype=np.uint64)) * 2 + 1 for _ in range(300)]
    assert all(v & 1 and 0 < v < 2**43 for v in vals)
    for pat in range(64):
        neg = [(pat >> i) & 1 for i in range(6)]
        for m in (vals[:6], vals[1:7], [1] * 6, [2**43 - 1] * 6, [1, 2**43 - 1] * 3, [2**43 - 1, 1] * 3):
            assert _resum(_recode(emu, m, neg)) == [(-v if s else v) for v, s in zip(m, neg)], (pat, m)
    for t in range(6, len(vals) - 5, 6):
        m = vals[t:t + 6]; neg = [int(x) for x in rng.integers(0, 2, 6)]
        assert _resum(_recode(emu, m, neg)) == [(-v if s else v) for v, s in zip(m, neg)], m


def _halves_back(tot):
    return [tot[hf] + 2**43 * tot[2 + hf] + 2**86 * tot[4 + hf] for hf in range(2)]


def test_fields_give_back_both_halves(emu):
    """the 43 fields of a step, summed over the levels on the bases 1, 2^43, 2^86, are the two signed GLV halves: the split-bound scalars of
    the step list, random e, random halves, and halves given directly whose upper pieces are all even (both borrows of sc_split_pieces3
    taken), all odd (none) and mixed, at both signs"""
    rng = np.random.default_rng(9702)
    es = list(split_bound_scalars()) + [int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1 for _ in range(200)]
    for e in es:
        m = (U64 * 6)(); neg = (ctypes.c_int * 6)(); hw = (ctypes.c_uint32 * 10)(); hn = (ctypes.c_int * 2)()
        emu.emu_r3_pieces(m, neg, hw, hn, b32(e % N))
        halves = [(-1 if hn[hf] else 1) * sum(hw[5 * hf + i] << (32 * i) for i in range(5)) for hf in range(2)]
        assert all(v & 1 and v < 2**43 for v in m)
        assert _halves_back(_resum(_recode(emu, list(m), list(neg)))) == halves, hex(e)
        assert (halves[0] + LAMBDA * halves[1]) % N == e % N
    mk = lambda p0, p1, p2: p0 + 2**43 * p1 + 2**86 * p2
    top = 2**43 - 1
    given = [mk(1, 0, 0), mk(1, 0, 2), mk(top, 0, top - 1), mk(1, 2, 4), mk(top, top - 1, top - 1),          # upper pieces all even
             mk(1, 1, 1), mk(top, top, top), mk(5, 3, 2**42 + 1), mk(top, top, 1),                            # upper pieces all odd
             mk(1, 0, 1), mk(1, 1, 0), mk(top, top, 0), mk(3, top - 1, top), 2**129 - 1, 2**128 + 1, 1]       # mixed, and the ends of the range
    given += [int.from_bytes(bytes(rng.integers(0, 256, 17, dtype=np.uint8)), "big") % 2**129 | 1 for _ in range(100)]
    for n, h in enumerate(given):
        for s0, s1 in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            halves = [s0 * h, s1 * given[(n + 3) % len(given)]]
            hw = (ctypes.c_uint32 * 10)(*[(abs(x) >> (32 * i)) & 0xFFFFFFFF for x in halves for i in range(5)])
            hn = (ctypes.c_int * 2)(*[int(x < 0) for x in halves])
            m = (U64 * 6)(); neg = (ctypes.c_int * 6)()
            emu.emu_r3_pieces_of_halves(m, neg, hw, hn)
            assert all(v & 1 and v < 2**43 for v in m), [hex(x) for x in halves]
            assert _halves_back(_resum(_recode(emu, list(m), list(neg)))) == halves, [hex(x) for x in halves]


def sector_multiplier(sector):
    """the multiplier of C that the entry at `sector` holds: the six digits of field 0 << 5 | sector on their bases"""
    return sum(d * k for d, k in zip(_digits(sector), BASE_K)) % N


def _table_points(ref):
    rng = np.random.default_rng(9704)
    g = np.frombuffer(G_XY, np.uint8)
    g2, _ = ref.ecmult_batch(g.reshape(1, 64), np.frombuffer(b32(2), np.uint8).reshape(1, 32))
    pts = [g, g2[0]] + [np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(8)]
    return pts + [np.frombuffer(c, np.uint8) for _, c in _golden_small_x_points()[:4]]


def test_every_table_entry(emu, ref):
    """all 32 sectors, taken back to the real curve with the Z factor, equal (1 +- 2^43 +- 2^86 +- lambda +- lambda 2^43 +- lambda 2^86) C
    by the reference: G, 2G, eight random points and the points with x below 2^32 that tests/golden holds"""
    ks = np.stack([np.frombuffer(b32(sector_multiplier(sector)), np.uint8) for sector in range(32)])
    assert len({k.tobytes() for k in ks}) == 32
    for c in _table_points(ref):
        out = ctypes.create_string_buffer(2048)
        assert emu.emu_r6_table(out, c.tobytes(), PARK_WORDS) == 1
        want, winf = ref.ecmult_batch(np.tile(c, (32, 1)), ks)
        assert not winf.any() and out.raw == want.tobytes()


def test_step_list(emu, steps):
    """every step equals the reference's and the three-base form's (with the caller's fallback where one hands back); no random triple
    hands back, a listed multiplier only where tests/ring_triple_cases.py names it (none is named: every listed multiplier completes)"""
    C, e, s, f, kinds, want = steps
    back = []
    for i in range(len(e)):
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        inf = emu.emu_r6_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 0, PARK_WORDS)
        assert inf == 0 and out.raw == want[i].tobytes(), (i, kinds[i])
        out3 = ctypes.create_string_buffer(64); took3 = ctypes.c_int(-1)
        assert emu.emu_r3_step(out3, ctypes.byref(took3), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 0) == 0
        assert out3.raw == out.raw, (i, kinds[i])
        if not took.value:
            back.append((kinds[i], int.from_bytes(e[i].tobytes(), "big")))
    assert not [k for k in back if k[0] != "listed"], back
    assert len(HANDBACK_ALLOWED) <= 2 and {v for _, v in back} <= set(HANDBACK_ALLOWED), back


def test_zero_z_factor_hands_back(emu, steps):
    """a table whose Z factor is zero (what a dx of zero in the construction leaves) makes the step return 0; the fallback gives the result"""
    C, e, s, f, kinds, want = steps
    for i in [k for k, kind in enumerate(kinds) if kind == "random"][:4]:
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        assert emu.emu_r6_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 1, PARK_WORDS) == 0
        assert took.value == 0 and out.raw == want[i].tobytes()


def _mul_g(ref, ks):
    g = np.tile(np.frombuffer(G_XY, np.uint8), (len(ks), 1))
    out, inf = ref.ecmult_batch(g, np.stack([np.frombuffer(b32(k % N), np.uint8) for k in ks]))
    assert not inf.any()
    return out


def zero_dx_cases(ref):
    """(name, (C, T1, T2) as (3, 64) points) with t1, t2 (and c) random multipliers of G: one dx of the construction vanishes in each; and the
    three free points themselves, where none does"""
    rng = np.random.default_rng(9705)
    r = lambda: int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1
    c, t1, t2 = r(), r(), r()
    inv = lambda v: pow(v % N, -1, N)
    cases = [
        ("batch 1: C = T1", (t1, t1, t2)),
        ("batch 1: C = -T1", (N - t1, t1, t2)),
        ("batch 2, pair 0: T2 = C + T1", (c, t1, c + t1)),
        ("batch 2, pair 1: T2 = -(C - T1)", (c, t1, t1 - c)),
        ("batch 3, pair 1: A_0 = lambda A_1", ((LAMBDA * (t2 - t1) - t1 - t2) * inv(1 - LAMBDA), t1, t2)),
        ("batch 3, pair 6: A_1 = lambda A_2", ((t1 - t2) * (1 + LAMBDA) * inv(1 - LAMBDA), t1, t2)),
        ("batch 3, pair 12: A_3 = -lambda A_0", ((t1 + t2) * (1 - LAMBDA) * inv(1 + LAMBDA), t1, t2)),
    ]
    pts = _mul_g(ref, [k for _, ks in cases for k in ks]).reshape(len(cases), 3, 64)
    return [(name, p) for (name, _), p in zip(cases, pts)], _mul_g(ref, [c, t1, t2])


def test_a_zero_dx_zeroes_the_z_factor(emu, ref):
    """in each of the three batches: the Z factor normalises to zero and a step on that table returns 0; three bases with nothing coinciding
    give a Z factor that is not zero and a step that completes"""
    cases, free = zero_dx_cases(ref)
    rng = np.random.default_rng(9706)
    e, s, f = (bytes(rng.integers(0, 128, 32, dtype=np.uint8)) for _ in range(3))
    r64 = ctypes.create_string_buffer(64)
    for name, p in cases:
        words = np.zeros(520, np.uint32)
        ok = emu.emu_r6_table_words(words.ctypes.data, p[0].tobytes(), p[1].tobytes(), p[2].tobytes(), PARK_WORDS)
        assert ok == 0 and not words[512:].any(), name
        assert emu.emu_r6_step_bases(r64, p[0].tobytes(), p[1].tobytes(), p[2].tobytes(), e, s, f, PARK_WORDS) == 0, name
    words = np.zeros(520, np.uint32)
    assert emu.emu_r6_table_words(words.ctypes.data, free[0].tobytes(), free[1].tobytes(), free[2].tobytes(), PARK_WORDS) == 1 and words[512:].any()
    assert emu.emu_r6_step_bases(r64, free[0].tobytes(), free[1].tobytes(), free[2].tobytes(), e, s, f, PARK_WORDS) == 1


def test_parking_map_fits_under_the_address_sanitizer():
    """tests/host_emul/ring_six_bounds (its own main, -fsanitize=address,undefined, runtimes linked statically): a table of exactly 528 and
    a parking area of exactly W = 243 words, both on the heap; the construction and four steps against the general form"""
    prog = os.path.join(HERE, "host_emul", "ring_six_bounds")
    assert os.path.exists(prog), "tests/host_emul/ring_six_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
