"""CPU tier: the signed-accumulator forms of the six-base ring step (csrc/group.h: gej_dblneg_ring, gej_rsub_ge_ring, gez_add_ge_ring) on
the host (tests/host_emul/ring_step_trim_emu.cpp, S2K_VERIFY on: a limb that would wrap aborts the process), each against the shared lean
form it replaces, equal after full normalisation: every limb at the contract's maximum for the coordinate's entry magnitude, 0, 1 and p - 1
in each coordinate, random values.  Then the forms where the kernel uses them: the chain of rp_rings_shared, the step list of
tests/ring_joint_cases.py through the step that returns its point as fractions, against the unmodified reference; an operand with the
accumulator's own x at the first, a middle and the last variable-part addition; and a step with a heap digit area of exactly its declared
size under the address sanitizer.
Not here: the digit records of the issue.  The word walk of the variable part was built and taken out again -- the static count of the
level body went from 2 704 to 2 710 VALU instructions with it (6 scalar instructions fewer): the index arithmetic it removes is scalar
already -- and one record per table-part addition does not fit: G and the generator want 2 x W = 20 records at D = 26 and 26 at D = 20,
the digit area has 18 words beside the nine field words.  op_locate and gtab_locate are what they were; tests/test_cpu_ring_six.py covers them."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests.refapi import N
from tests.ring_joint_cases import b32, reference, step_list
from tests.test_cpu_oracle import LAMBDA
from tests.test_cpu_ring_six import LEVELS, PARK_WORDS, _digits, _mul_g, _recode

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2**256 - 2**32 - 977
U64 = ctypes.c_ulonglong


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_step_trim_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_step_trim_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_trim_dbl.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
    lib.emu_trim_rsub.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.emu_trim_gez.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.emu_trim_step_bases.argtypes = [ctypes.c_char_p] * 7 + [ctypes.c_int]
    lib.emu_trim_step.argtypes = [ctypes.c_char_p] * 5 + [ctypes.c_int]
    return lib


def limbs(v):
    """a value below 2^256 as nine 29-bit limbs"""
    return [(v >> (29 * i)) & (2**29 - 1) for i in range(9)]


def limbs_max(m):
    """every limb at the largest value the contract of csrc/fe.h allows at magnitude m"""
    return [m * (2**29 + 2**20)] * 8 + [m * (2**24 + 2**10)]


# entry magnitudes of the coordinates, in the order the wrappers take them (csrc/group.h, the comment above each form)
FORMS = {
    "dbl": (1, 2, 1),                   # x (holds +X), y, z
    "dbl_nx": (2, 2, 1),                # x (holds -X), y, z
    "rsub": (1, 1, 1, 1, 2),            # x, y, z, operand x, operand y
    "gez": (2, 1, 1, 1, 1, 2),          # x, y, zz, zzz, operand x, operand y
}


def form_cases(name):
    """rows of raw limbs: all coordinates at their maximum; each coordinate in turn at its maximum, 0, 1, p - 1 among random canonical
    values; every coordinate 0 / 1 / p - 1 at once; random canonical rows.  Shared by the CPU and the GPU tier."""
    mags = FORMS[name]
    rng = np.random.default_rng(9950 + len(mags) + sum(mags))
    rnd = lambda: limbs(int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % P)
    rows = [[limbs_max(m) for m in mags]]
    for k, m in enumerate(mags):
        for special in (limbs_max(m), limbs(0), limbs(1), limbs(P - 1)):
            rows.append([special if i == k else rnd() for i in range(len(mags))])
    for v in (0, 1, P - 1):
        rows.append([limbs(v) for _ in mags])
    for pair in itertools.product((limbs(1), limbs(P - 1)), repeat=2):
        rows.append([pair[i & 1] for i in range(len(mags))])
    rows += [[rnd() for _ in mags] for _ in range(16)]
    return np.array(rows, np.uint32).reshape(len(rows), 9 * len(mags))


def run_form(emu, name, row):
    """-> (the new form's result limb for limb, what it stands for || the shared form's result as canonical bytes, flag)"""
    n_out = 36 if name == "gez" else 27
    out = np.zeros(n_out, np.uint32); cmp_ = ctypes.create_string_buffer(2 * 32 * (n_out // 9))
    row = np.ascontiguousarray(row, np.uint32)
    flag = 0
    if name in ("dbl", "dbl_nx"):
        emu.emu_trim_dbl(out.ctypes.data, cmp_, row.ctypes.data, int(name == "dbl_nx"))
    elif name == "rsub":
        flag = emu.emu_trim_rsub(out.ctypes.data, cmp_, row.ctypes.data)
    else:
        emu.emu_trim_gez(out.ctypes.data, cmp_, row.ctypes.data)
    return out, cmp_.raw, flag


@pytest.mark.parametrize("name", list(FORMS))
def test_form_equals_the_shared_form(emu, name):
    for k, row in enumerate(form_cases(name)):
        out, raw, flag = run_form(emu, name, row)
        half = len(raw) // 2
        assert raw[:half] == raw[half:], (name, k)
        assert flag in (0, 3), (name, k, flag)                  # the same-x verdict of the new form is the shared form's
        # exit magnitudes as the comments state them: 1 everywhere but the XYZZ form's x (2)
        for c in range(len(out) // 9):
            m = 2 if (name == "gez" and c == 0) else 1
            assert (out[9 * c:9 * c + 9] <= np.array(limbs_max(m), np.uint64)).all(), (name, k, c)


def test_same_x_is_reported_by_the_new_addition(emu):
    """operand x * Z^2 == X: the flag is set by both forms, whatever the y"""
    z = 0x1234567; x2 = 0xABCDEF12345
    row = [limbs(x2 * z * z % P), limbs(5), limbs(z), limbs(x2), limbs(7)]
    _, _, flag = run_form(emu, "rsub", np.array(row, np.uint32).reshape(-1))
    assert flag == 3


def test_chain_is_the_doublings(emu, ref):
    rng = np.random.default_rng(9951)
    for _ in range(3):
        c = ref.rand_point(rng)
        t1 = ctypes.create_string_buffer(64); t2 = ctypes.create_string_buffer(64)
        assert emu.emu_trim_chain(t1, t2, c) == 0
        want, inf = ref.ecmult_batch(np.frombuffer(c * 2, np.uint8).reshape(2, 64), np.stack([np.frombuffer(b32(2**43), np.uint8), np.frombuffer(b32(2**86), np.uint8)]))
        assert not inf.any() and t1.raw == want[0].tobytes() and t2.raw == want[1].tobytes()


def test_step_list_as_fractions(emu, ref):
    """every step of the list completes on the new forms and, taken to affine from the fractions, is the reference's point"""
    C, e, s, f, kinds = step_list(ref)
    want, winf = reference(ref, C, e, s, f)
    assert not winf.any()
    for i in range(len(kinds)):
        out = ctypes.create_string_buffer(64)
        assert emu.emu_trim_step(out, C[i].tobytes(), e[i].tobytes(), s[i].tobytes(), f[i].tobytes(), PARK_WORDS) == 1, (i, kinds[i])
        assert out.raw == want[i].tobytes(), (i, kinds[i])


def _level_forms(emu6, e):
    """the operand of each level as a linear form over (c, t1, t2) mod n, from the step's own digit words"""
    m = (U64 * 6)(); neg = (ctypes.c_int * 6)(); hw = (ctypes.c_uint32 * 10)(); hn = (ctypes.c_int * 2)()
    emu6.emu_r3_pieces(m, neg, hw, hn, b32(e))
    dw = _recode(emu6, list(m), list(neg))
    forms = []
    for level in range(LEVELS):
        d = _digits((dw[level // 5] >> ((level % 5) * 6)) & 63)
        forms.append(tuple((d[2 * b] + LAMBDA * d[2 * b + 1]) % N for b in range(3)))
    return forms


@pytest.mark.parametrize("level,sign", [(1, 1), (21, -1), (LEVELS - 1, 1), (LEVELS - 1, -1)])
def test_same_x_in_the_variable_part_hands_back(emu, ref, level, sign):
    """bases c G, t1 G, t2 G with c solved so that twice the accumulator in front of `level` is +-(that level's operand): the step returns 0;
    with c free it completes"""
    emu6 = ctypes.CDLL(os.path.join(HERE, "host_emul", "libs2k_ring_six_emu.so"))
    rng = np.random.default_rng(9952 + level)
    r = lambda: int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1
    e, t1, t2, c_free = r(), r(), r(), r()
    forms = _level_forms(emu6, e)
    acc = (0, 0, 0)
    for lv in range(level):
        acc = tuple((2 * a + o) % N for a, o in zip(acc, forms[lv]))
    lin = tuple((2 * a - sign * o) % N for a, o in zip(acc, forms[level]))       # 2 acc -+ operand, as a form over (c, t1, t2)
    assert lin[0] % N
    c = -(lin[1] * t1 + lin[2] * t2) * pow(lin[0], -1, N) % N
    assert c and (lin[0] * c + lin[1] * t1 + lin[2] * t2) % N == 0
    # no earlier level meets its operand's x with this c
    a = 0
    for lv in range(level):
        o = (forms[lv][0] * c + forms[lv][1] * t1 + forms[lv][2] * t2) % N
        assert lv == 0 or ((2 * a - o) % N and (2 * a + o) % N)
        a = (2 * a + o) % N
    s, f = (bytes(rng.integers(0, 128, 32, dtype=np.uint8)) for _ in range(2))
    pts = _mul_g(ref, [c, t1, t2, c_free])
    r64 = ctypes.create_string_buffer(64)
    assert emu.emu_trim_step_bases(r64, pts[0].tobytes(), pts[1].tobytes(), pts[2].tobytes(), b32(e), s, f, PARK_WORDS) == 0
    assert emu.emu_trim_step_bases(r64, pts[3].tobytes(), pts[1].tobytes(), pts[2].tobytes(), b32(e), s, f, PARK_WORDS) == 1
    sf = (int.from_bytes(s, "big") + int.from_bytes(f, "big")) % N
    want = _mul_g(ref, [(forms_total(forms, c_free, t1, t2) + sf) % N])
    assert r64.raw == want[0].tobytes()


def forms_total(forms, c, t1, t2):
    a = 0
    for o in forms:
        a = (2 * a + o[0] * c + o[1] * t1 + o[2] * t2) % N
    return a


def test_digit_area_of_exactly_its_size_under_the_address_sanitizer():
    """tests/host_emul/ring_step_trim_bounds (its own main, -fsanitize=address,undefined, runtimes linked statically): table, parking area
    and the 27-word digit area on the heap at exactly their declared sizes; three steps on the new forms against the general form"""
    prog = os.path.join(HERE, "host_emul", "ring_step_trim_bounds")
    assert os.path.exists(prog), "tests/host_emul/ring_step_trim_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
