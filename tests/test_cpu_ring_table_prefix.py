"""CPU tier: the construction of the three-base ring table (csrc/ecmult.h: ecmult_ring3_tables, prefix products of the dx formed from the
parked inputs alone, every conjugate pair added once) on the host with C, T1 and T2 given independently
(tests/host_emul/ring_table_prefix_emu.cpp): honest inputs against the words recorded from the construction that parked both sums of every
pair (tests/golden/ring_table_prefix.npz), a dx of zero at every place the prefix chain can break, and the compact parking map's bounds
under the address sanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.refapi import G_XY, N
from tests.ring_joint_cases import b32, split_bound_scalars

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ring_table_prefix.npz")
PARK_WORDS = 414                                      # W: highest used word + 1 of a lane's parking map (csrc/ecmult.h, above piece43)
INV3 = pow(3, -1, N)


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_table_prefix_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_table_prefix_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_r3p_table.argtypes = [ctypes.c_void_p] + [ctypes.c_char_p] * 3 + [ctypes.c_int]
    lib.emu_r3p_step.argtypes = [ctypes.c_char_p] * 7 + [ctypes.c_int]
    return lib


def _mul_g(ref, ks):
    """k*G for every k of the list -> (len, 64) uint8"""
    g = np.tile(np.frombuffer(G_XY, np.uint8), (len(ks), 1))
    out, inf = ref.ecmult_batch(g, np.stack([np.frombuffer(b32(k % N), np.uint8) for k in ks]))
    assert not inf.any()
    return out


def honest_bases(ref):
    """(n, 3, 64): C, 2^43 C, 2^86 C for C = G, 2G, six random points and k*G for the twenty split-bound scalars of tests/golden"""
    rng = np.random.default_rng(9600)
    ks = [1, 2] + [int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1 for _ in range(6)] + list(split_bound_scalars()[:20])
    return np.stack([_mul_g(ref, ks), _mul_g(ref, [k << 43 for k in ks]), _mul_g(ref, [k << 86 for k in ks])], axis=1)


def table(emu, bases, park_words=PARK_WORDS):
    """-> (520 words: 32 sectors + the normalised Z factor, 1 when the Z factor is not zero)"""
    out = np.zeros(520, np.uint32)
    ok = emu.emu_r3p_table(out.ctypes.data, bases[0].tobytes(), bases[1].tobytes(), bases[2].tobytes(), park_words)
    return out, ok


def record(ref, emu, path=GOLDEN):
    """writes the fixture: run on the commit BEFORE the construction changed (park_words = 864, the whole area it used)"""
    bases = honest_bases(ref)
    words = np.stack([table(emu, b, 864)[0] for b in bases])
    np.savez_compressed(path, bases=bases, words=words)


def test_honest_tables_equal_the_recorded_words(emu):
    """all 32 sectors and the Z factor, word for word, are what the parent commit's host build gave for the same 28 triples"""
    gold = np.load(GOLDEN)
    assert gold["bases"].shape == (28, 3, 64) and gold["words"].shape == (28, 520)
    for i, (b, want) in enumerate(zip(gold["bases"], gold["words"])):
        got, ok = table(emu, b)
        assert ok == 1 and want[512:].any(), i
        assert np.array_equal(got, want), (i, np.nonzero(got != want)[0][:8])


def test_recorded_inputs_are_the_named_points(ref):
    assert np.array_equal(np.load(GOLDEN)["bases"], honest_bases(ref))


def test_recorded_tables_hold_the_multiples(ref):
    """the recorded sectors, taken back to the real curve with the recorded Z factor, are (a + b 2^43 + c 2^86) C: checked on G and 2G
    through X = x / Z^2 compared crosswise, x_sector == X_ref * Z^2 (mod p)"""
    P = 2**256 - 2**32 - 977
    gold = np.load(GOLDEN)
    for i in range(2):
        w = gold["words"][i]
        z = sum(int(v) << (32 * k) for k, v in enumerate(w[512:]))
        ks = []
        for sector in range(32):
            a, b, c = 2 * (sector >> 4) + 1, 2 * ((sector >> 2) & 3) - 3, 2 * (sector & 3) - 3
            ks.append((i + 1) * (a + b * 2**43 + c * 2**86) % N)
        want = _mul_g(ref, ks)
        for sector in range(32):
            x = sum(int(v) << (32 * k) for k, v in enumerate(w[16 * sector:16 * sector + 8]))
            y = sum(int(v) << (32 * k) for k, v in enumerate(w[16 * sector + 8:16 * sector + 16]))
            X = int.from_bytes(want[sector, :32].tobytes(), "big"); Y = int.from_bytes(want[sector, 32:].tobytes(), "big")
            assert x == X * z * z % P and y == Y * z * z * z % P, (i, sector)


def _zero_dx_cases(ref):
    """(name, (C, T1, T2)) with t1, t2 random: one dx of the construction vanishes in each"""
    rng = np.random.default_rng(9601)
    r = lambda: int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1
    c, t1, t2 = r(), r(), r()
    cases = [
        ("stage 1, pairs 0 and 3: T2 = T1", (c, t1, t1)),
        ("stage 1, pairs 0 and 3: T2 = -T1", (c, t1, N - t1)),
        ("stage 2, pair 0: C = T1 + T2", (t1 + t2, t1, t2)),
        ("stage 2, pair 0: C = -(T1 + T2)", (N - (t1 + t2) % N, t1, t2)),
        ("stage 2, pair 7: C = 3 T1 - 3 T2", (3 * (t1 - t2), t1, t2)),
        ("stage 2, pair 8: 3 C = T1 + T2", ((t1 + t2) * INV3, t1, t2)),
        ("stage 2, pair 15 (and 1): 3 C = 3 T1 - 3 T2", (t1 - t2, t1, t2)),
    ]
    pts = _mul_g(ref, [k for _, ks in cases for k in ks]).reshape(len(cases), 3, 64)
    free = _mul_g(ref, [c, t1, t2])
    return [(name, p) for (name, _), p in zip(cases, pts)], free


def test_a_zero_dx_zeroes_the_z_factor(emu, ref):
    """each time the Z factor normalises to zero and a step on that table returns 0; the same three scalars with nothing coinciding
    give a table whose step completes with e*C + (s + f)*G"""
    cases, free = _zero_dx_cases(ref)
    rng = np.random.default_rng(9602)
    e, s, f = (bytes(rng.integers(0, 128, 32, dtype=np.uint8)) for _ in range(3))
    r64 = ctypes.create_string_buffer(64)
    for name, p in cases:
        words, ok = table(emu, p)
        assert ok == 0 and not words[512:].any(), name
        assert emu.emu_r3p_step(r64, p[0].tobytes(), p[1].tobytes(), p[2].tobytes(), e, s, f, PARK_WORDS) == 0, name
    # control: independent bases do not form a table of one point, so only its Z factor and completion are looked at here ...
    words, ok = table(emu, free)
    assert ok == 1 and words[512:].any()
    # ... and an honest triple completes with the reference's result
    gold = np.load(GOLDEN)
    b = gold["bases"][3]
    assert emu.emu_r3p_step(r64, b[0].tobytes(), b[1].tobytes(), b[2].tobytes(), e, s, f, PARK_WORDS) == 1
    sf = (int.from_bytes(s, "big") + int.from_bytes(f, "big")) % N
    want, inf = ref.ecmult_batch(b[0].reshape(1, 64), np.frombuffer(e, np.uint8).reshape(1, 32), ng=np.frombuffer(b32(sf), np.uint8).reshape(1, 32))
    assert not inf.any() and r64.raw == want[0].tobytes()


def test_compact_map_fits_under_the_address_sanitizer():
    """tests/host_emul/ring_table_prefix_bounds (its own main, -fsanitize=address,undefined, runtimes linked statically): a table of exactly
    528 and a parking area of exactly W = 414 words, both on the heap; the construction and four steps against the general form"""
    prog = os.path.join(HERE, "host_emul", "ring_table_prefix_bounds")
    assert os.path.exists(prog), "tests/host_emul/ring_table_prefix_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
