"""CPU tier: the ring form of secp256k1_zkp_amd/csrc/ecmult.h with its joint table (one table indexed by the digits of C and of T = 2^64 C,
S2K_RING_JOINT = 1) on the host (tests/host_emul/ring_joint_emu.cpp, S2K_VERIFY on): the recoding on integers, every table entry and the
step list against the unmodified reference; the same step list through the build with -DS2K_RING_JOINT=0 (two separate tables) as control."""
import ctypes
import os

import numpy as np
import pytest

from tests.refapi import G_XY, N
from tests.ring_joint_cases import HANDBACK_ALLOWED, b32, reference, step_list

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    path = os.path.join(HERE, "host_emul", name)
    assert os.path.exists(path), f"tests/host_emul/{name} not built (python -c 'import __graft_entry__ as g; g.build()')"
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def emu():
    lib = _load("libs2k_ring_joint_emu.so")
    assert lib.emu_rj_joint() == 1 and lib.emu_rj_adds() == 44
    return lib


@pytest.fixture(scope="module")
def emu0():
    lib = _load("libs2k_ring_joint0_emu.so")
    assert lib.emu_rj_joint() == 0 and lib.emu_rj_adds() == 52
    return lib


@pytest.fixture(scope="module")
def steps(ref):
    C, e, s, f, kinds = step_list(ref)
    want, winf = reference(ref, C, e, s, f)
    assert not winf.any()
    return C, e, s, f, kinds, want


def _pieces():
    rng = np.random.default_rng(9101)
    vals = [1, 3, 2**63 - 1, 2**63 + 1, 2**64 - 1, 2**64 + 1, 2**65 - 1, int("5" * 16, 16), int("5" * 16, 16) | 2**64, int("A" * 16, 16) | 1, (int("A" * 16, 16) | 1) | 2**64]
    vals += [int.from_bytes(bytes(rng.integers(0, 256, 9, dtype=np.uint8)), "little") % 2**65 | 1 for _ in range(200)]
    assert all(v & 1 and v < 2**65 for v in vals)
    return vals


def _words(v):
    return (ctypes.c_uint32 * 3)(v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, v >> 64)


def _digits(emu, v):
    out = (ctypes.c_int * 22)()
    emu.emu_rj_piece_digits(out, _words(v))
    return list(out)


def test_sizes_the_yardsticks_pin(emu, emu0):
    for lib in (emu, emu0):
        out = (ctypes.c_int * 4)()
        lib.emu_rj_sizes(out)
        assert list(out) == [528, 2 * 16 * 27 * 64, 2 * 16 * 27, 27]


def test_digits_resum_to_the_piece(emu):
    for v in _pieces():
        d = _digits(emu, v)
        assert all(x in (-7, -5, -3, -1, 1, 3, 5, 7) for x in d)
        assert sum(x * 8**i for i, x in enumerate(d)) == v, hex(v)


def test_field_selects_the_signed_pair(emu):
    """every (field of the C piece, field of the T piece, sign of the C piece, sign of the T piece): neg << 5 | sector with sector =
    ((a - 1) / 2) * 8 + (b + 7) / 2 selects +-J(a, b) = +-(a C + b T) whose C and T multipliers are the signed digits"""
    seen = set()
    for vc in range(8):
        for vt in range(8):
            for sc in (0, 1):
                for st in (0, 1):
                    dc = (2 * vc - 7) * (-1 if sc else 1); dt = (2 * vt - 7) * (-1 if st else 1)
                    fld = emu.emu_rj_field(vc, vt, sc, st)
                    assert 0 <= fld < 64
                    sign = -1 if fld >> 5 else 1
                    a = 2 * ((fld >> 3) & 3) + 1; b = 2 * (fld & 7) - 7
                    assert (sign * a, sign * b) == (dc, dt), (vc, vt, sc, st)
                    seen.add(fld)
    assert len(seen) == 64


def test_recode_words_hold_the_fields_of_the_four_pieces(emu):
    """the nine digit words of a step: field (level * 2 + half), five to a word, for pieces with both signs; summed back over the levels
    the selected multiples are the signed pieces"""
    pcs = _pieces()
    rng = np.random.default_rng(9102)
    for t in range(0, len(pcs) - 3, 2):
        p = pcs[t:t + 4]; neg = [int(x) for x in rng.integers(0, 2, 4)]
        if t < 16:
            neg = [(t >> 1) & 1, (t >> 2) & 1, (t >> 3) & 1, 1 - ((t >> 1) & 1)]
        w12 = (ctypes.c_uint32 * 12)(*[x for v in p for x in _words(v)]); n4 = (ctypes.c_int * 4)(*neg); dw = (ctypes.c_uint32 * 9)()
        emu.emu_rj_recode(dw, w12, n4)
        tot = [0, 0, 0, 0]
        for idx in range(44):
            fld = (dw[idx // 5] >> ((idx % 5) * 6)) & 63
            level, hf = idx >> 1, idx & 1
            sign = -1 if fld >> 5 else 1
            a = sign * (2 * ((fld >> 3) & 3) + 1); b = sign * (2 * (fld & 7) - 7)
            tot[hf] += a * 8**(21 - level); tot[2 + hf] += b * 8**(21 - level)
        assert tot == [(-v if s else v) for v, s in zip(p, neg)]
        assert dw[8] >> 24 == 0                                  # 44 fields: the 45th place stays clear


def _table_points(ref):
    rng = np.random.default_rng(9103)
    g = np.frombuffer(G_XY, np.uint8)
    g2, _ = ref.ecmult_batch(g.reshape(1, 64), np.frombuffer(b32(2), np.uint8).reshape(1, 32))
    return [g, g2[0]] + [np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(8)]


def _golden_small_x_points():
    """every point with x below 2^32 that a text file under tests/golden holds as hex: x | y (64 bytes) or compressed (02 / 03 and x)"""
    import re
    from tests.refapi import P
    found = []
    gdir = os.path.join(HERE, "golden")
    for root, _, files in os.walk(gdir):
        for name in sorted(files):
            try:
                text = open(os.path.join(root, name), encoding="utf-8").read()
            except (UnicodeDecodeError, OSError):
                continue
            for m in re.finditer(r"(?<![0-9a-fA-F])(0[23])?(0{56}[0-9a-fA-F]{8})([0-9a-fA-F]{64})?(?![0-9a-fA-F])", text):
                x = int(m.group(2), 16); rhs = (x * x * x + 7) % P
                if m.group(1) and not m.group(3):
                    y = pow(rhs, (P + 1) // 4, P)
                    if y * y % P != rhs:
                        continue
                    if (y & 1) != (int(m.group(1), 16) & 1):
                        y = P - y
                elif m.group(3) and not m.group(1):
                    y = int(m.group(3), 16)
                    if y >= P or y * y % P != rhs:
                        continue
                else:
                    continue
                found.append((name, x.to_bytes(32, "big") + y.to_bytes(32, "big")))
    return found


def _check_table(emu, ref, c):
    out = ctypes.create_string_buffer(2048)
    assert emu.emu_rj_table(out, c.tobytes()) == 1
    ks = [b32(((2 * (sector >> 3) + 1) + (2 * (sector & 7) - 7) * 2**64) % N) for sector in range(32)]
    want, winf = ref.ecmult_batch(np.tile(c, (32, 1)), np.stack([np.frombuffer(k, np.uint8) for k in ks]))
    assert not winf.any() and out.raw == want.tobytes()


def test_table_of_a_golden_point_with_small_x(emu, ref):
    """a point with x below 2^32, where tests/golden holds one (searched above: every text file, hex x | y and compressed forms)"""
    pts = _golden_small_x_points()
    if not pts:
        pytest.skip("no file under tests/golden holds a point with x below 2^32")
    for _, c in pts[:4]:
        _check_table(emu, ref, np.frombuffer(c, np.uint8))


def test_every_table_entry(emu, ref):
    """all 32 sectors, taken back to the real curve with the Z factor, equal a C + b 2^64 C"""
    for c in _table_points(ref):
        _check_table(emu, ref, c)


def _run_steps(lib, steps):
    C, e, s, f, kinds, want = steps
    back = []
    for i in range(len(e)):
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        inf = lib.emu_rj_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 0)
        assert inf == 0 and out.raw == want[i].tobytes(), (i, kinds[i])          # with the caller's fallback wherever the step handed back
        if not took.value:
            back.append((kinds[i], int.from_bytes(e[i].tobytes(), "big")))
    return back


def _check_handbacks(back):
    assert not [k for k in back if k[0] == "random"], back
    listed = [v for k, v in back if k == "listed"]
    assert len(listed) <= 2 and set(listed) <= set(HANDBACK_ALLOWED), back


def test_step_list_joint_form(emu, steps):
    _check_handbacks(_run_steps(emu, steps))


def test_step_list_separate_form_as_control(emu0, steps):
    _check_handbacks(_run_steps(emu0, steps))


def test_zero_z_factor_hands_back(emu, steps):
    """a table whose Z factor is zero (what a dx of zero in the construction leaves) makes the step return 0; the fallback gives the result"""
    C, e, s, f, kinds, want = steps
    for i in [k for k, kind in enumerate(kinds) if kind == "random"][:4]:
        out = ctypes.create_string_buffer(64); took = ctypes.c_int(-1)
        assert emu.emu_rj_step(out, ctypes.byref(took), C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), 1) == 0
        assert took.value == 0 and out.raw == want[i].tobytes()
