"""CPU tier: ECDSA adaptor-signature verification and the two-point multiplication.  secp256k1_zkp_amd/csrc/adaptor.h and ecmult_lane2
(csrc/ecmult.h) run on the host (tests/host_emul/adaptor_emu.cpp, S2K_VERIFY on, 12-bit generator table) against the Python model of
tests/adaptor_ref.py and the recorded vectors (tests/golden/adaptor_vectors.json: the verdicts of the reference's own
secp256k1_ecdsa_adaptor_verify); the two-point multiplication against the reference's secp256k1_ecmult_multi_var with two terms; plus
the midstate, the ABI, the argument checks and the C example."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import adaptor_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADAPTOR_SYMBOLS = ["secp256k1_ecdsa_adaptor_verify_batch", "secp256k1_ecdsa_adaptor_verify_batch_dev", "secp256k1_ecdsa_adaptor_verify_batch_group",
                   "secp256k1_ecdsa_adaptor_verify_amd", "s2k_ecmult2_batch", "s2k_ecmult2_batch_dev"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_adaptor_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_adaptor_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_adaptor_verify.argtypes = [ctypes.c_char_p] * 4 + [ctypes.c_int]
    lib.emu_adaptor_joint_count.restype = ctypes.c_ulonglong
    lib.emu_ecmult2.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    lib.emu_adaptor_midstate.argtypes = [ctypes.c_char_p]
    lib.emu_adaptor_challenge.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib


def golden():
    return A.from_json(json.load(open(os.path.join(HERE, "golden", "adaptor_vectors.json")))["vectors"])


def _run_items(emu, items, formats=(0, 1, 2)):
    """every item through the host-emulated lane routine, in every key format it exists in"""
    ran = 0
    for it in items:
        for fmt in formats:
            keys = A.keys_in_format(it, fmt)
            if keys is None:
                continue
            assert emu.emu_adaptor_verify(it[1], keys[0], it[3], keys[1], fmt) == it[5], (it[0], fmt)
            ran += 1
    return ran


def test_golden_fixture_shape():
    v = golden()
    names = {x[0]: x for x in v}
    assert len(names) == len(v) and sum(1 for x in v if x[0].startswith("random ")) == 64
    assert [names["module vector %d" % i][5] for i in range(3)] == [1, 1, 0] and names["module issue 335: R1 at infinity"][5] == 0
    assert all(len(x[1]) == 162 and len(x[3]) == 32 for x in v)
    assert sum(1 for x in v if x[6] == 1) == 3 and all(x[5] == 0 for x in v if x[6] == 1)      # the all-zero objects: engine only
    rnd = [x for x in v if x[0].startswith("random ")]
    assert all(x[5] == 1 for i, x in enumerate(rnd) if i % 4 != 3) and all(x[5] == 0 for i, x in enumerate(rnd) if i % 4 == 3)


def test_model_against_fixture():
    """the Python model returns the reference's recorded verdict on every item the reference was asked"""
    for name, sig, pk, msg, ek, verdict, only in golden():
        if only is None:
            assert A.verify(sig, pk, msg, ek) == verdict, name


def test_edge_list_verdicts():
    """the edge list rebuilt now is the recorded one, and each item has the verdict its name promises"""
    cases = A.edge_cases()
    assert cases == [x for x in golden() if not x[0].startswith(("random ", "module "))]
    for it in cases:
        assert it[5] == A.EDGE_VERDICTS.get(it[0], 0), it[0]
    names = {x[0] for x in cases}
    assert set(A.EDGE_VERDICTS) <= names and len(names) == len(cases)
    for need in ("s' = 0", "s' = n", "s = n", "prefix 04 on R", "x >= p in R'", "s = 0", "e = 0", "n - s'", "R' negated", "R negated", "msg + 1", "Y negated",
                 "X negated", "X and Y swapped", "all-zero key objects", "s = e k: R1 at infinity", "R = k2 Y, s = e k2: R2 at infinity",
                 "R = k2 Y, s = -e k2: the doubling inside R2", "m = -sigr x: D at infinity", "m = sigr x: the doubling inside D"):
        assert need in names, need
    # s' + 1: the DLEQ half alone still passes (the proof does not cover s')
    it = next(x for x in cases if x[0].startswith("s' + 1"))
    f = A.sig_fields(it[1]); Rp, R, Y = A.parse33(f["Rp"]), A.parse33(f["R"]), A.parse33(it[4])
    R1 = A.pt_add(A.pt_mul(f["s"], A.G), A.pt_neg(A.pt_mul(f["e"], Rp))); R2 = A.pt_add(A.pt_mul(f["s"], Y), A.pt_neg(A.pt_mul(f["e"], R)))
    assert A.dleq_challenge(Rp, Y, R, R1, R2) == f["e"]


def test_model_group_law():
    """pt_mul (Jacobian) against repeated pt_add (affine), and the order of G"""
    acc = A.INF
    for k in range(1, 20):
        acc = A.pt_add(acc, A.G)
        assert A.pt_mul(k, A.G) == acc
    assert A.pt_mul(A.N, A.G) is A.INF and A.pt_mul(A.N - 1, A.G) == A.pt_neg(A.G)


def test_emu_golden(emu):
    """the recorded vectors in all three key formats (no reference needed)"""
    j0 = emu.emu_adaptor_joint_count()
    assert _run_items(emu, golden()) >= 3 * 90
    assert emu.emu_adaptor_joint_count() - j0 >= 100                                      # the joint form is what ordinary items take


def test_emu_fallback_items(emu):
    """items whose second point cannot go through the joint form (a zero scalar) take the two-call form: same verdicts, no joint run"""
    cases = {x[0]: x for x in A.edge_cases()}
    for name in ("s = 0", "e = 0", "s = n", "prefix 04 on R"):
        j0 = emu.emu_adaptor_joint_count()
        assert _run_items(emu, [cases[name]], formats=(0,)) == 1
        assert emu.emu_adaptor_joint_count() == j0, name


def test_emu_random_against_model(emu):
    """256 seeded items, one in four corrupted"""
    items = A.random_items(256, 5503)
    ones = sum(x[5] for x in items)
    assert ones >= 128 and 256 - ones >= 32
    _run_items(emu, items, formats=(0,))
    _run_items(emu, items[:32], formats=(1, 2))


def _xy(pt):
    return bytes(64) if pt is A.INF else pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def _ecmult2_cases():
    """(name, A, a_inf, na, B, b_inf, nb, expect_joint): expect_joint None where either form may serve the item"""
    rng = np.random.default_rng(5504)
    rs = lambda: A._rand_scalar(rng)                                                      # noqa: E731
    out = []
    for i in range(12):
        out.append((f"random {i}", A.pt_mul(rs(), A.G), 0, rs(), A.pt_mul(rs(), A.G), 0, rs(), 1))
    P, Q = A.pt_mul(rs(), A.G), A.pt_mul(rs(), A.G)
    for na in (0, 1, A.N - 1):
        for nb in (0, 1, A.N - 1):
            out.append((f"na = {na if na < 2 else 'n-1'}, nb = {nb if nb < 2 else 'n-1'}", P, 0, na, Q, 0, nb, 0 if 0 in (na, nb) else None))
    k = rs()
    for nm, B in (("A = B", P), ("A = -B", A.pt_neg(P))):
        out.append((nm + ", random scalars", P, 0, rs(), B, 0, rs(), None))
        out.append((nm + ", na = nb", P, 0, k, B, 0, k, None))                           # 2kP, or infinity
        out.append((nm + ", na = -nb", P, 0, k, B, 0, A.N - k, None))                     # infinity, or 2kP
    out.append(("A at infinity", P, 1, rs(), Q, 0, rs(), 0))
    out.append(("B at infinity", P, 0, rs(), Q, 1, rs(), 0))
    out.append(("both at infinity", P, 1, rs(), Q, 1, rs(), 0))
    # B = lambda^2 A = -(A + lambda A): the third addition of the joint form (top digit of B's first stream) can meet the accumulator's own x
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    for na, nb in ((1, 1), (3, 5), (rs(), rs())):
        out.append((f"B = lambda^2 A, na = {na:#x}, nb = {nb:#x}", P, 0, na, A.pt_mul(lam * lam % A.N, P), 0, nb, None))
    return out


def test_emu_ecmult2_against_model_and_reference(emu, ref):
    """na*A + nb*B from the joint form (or its fallback) against the plain-integer model and secp256k1_ecmult_multi_var with two terms"""
    took = {}
    for name, Pa, ainf, na, Pb, binf, nb, expect_joint in _ecmult2_cases():
        r = ctypes.create_string_buffer(b"\xff" * 64, 64); tj = ctypes.c_int(-1)
        inf = emu.emu_ecmult2(r, ctypes.byref(tj), _xy(Pa), ainf, A.b32(na), _xy(Pb), binf, A.b32(nb))
        want = A.pt_add(A.INF if ainf else A.pt_mul(na, Pa), A.INF if binf else A.pt_mul(nb, Pb))
        assert (inf, r.raw) == (int(want is A.INF), _xy(want)), name
        sc = np.frombuffer(A.b32(na) + A.b32(nb), np.uint8); pts = np.frombuffer(_xy(Pa) + _xy(Pb), np.uint8)
        rr, rinf = ref.ecmult_multi(sc, pts, pt_inf=np.array([ainf, binf], np.uint8))
        assert (int(rinf), bytes(rr) if not rinf else bytes(64)) == (inf, r.raw), name
        if expect_joint is not None:
            assert tj.value == expect_joint, name
        took[name] = tj.value
    assert sum(took.values()) >= 12 and any(v == 0 for v in took.values())


def test_midstate_and_challenge_against_hashlib(emu):
    """the midstate the engine computes with its own SHA-256 is the state after SHA256("DLEQ") twice, and the three-block challenge over
    it is SHA-256 of the full 229-byte message"""
    tag = hashlib.sha256(b"DLEQ").digest()
    mid = ctypes.create_string_buffer(32); emu.emu_adaptor_midstate(mid)
    # the reference keeps the same eight words as constants (src/modules/ecdsa_adaptor/dleq_impl.h:16-22); here they are derived, and
    # pinned through the digest below: a wrong midstate cannot give hashlib's digest of tag | tag | message
    rng = np.random.default_rng(5505)
    for _ in range(8):
        pts = b"".join(bytes([2 + int(rng.integers(0, 2))]) + bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()) for _ in range(5))
        e = ctypes.create_string_buffer(32); emu.emu_adaptor_challenge(e, pts)
        assert int.from_bytes(e.raw, "big") == int.from_bytes(hashlib.sha256(tag + tag + pts).digest(), "big") % A.N
    pts = b"".join(A.ser33(A.pt_mul(k, A.G)) for k in (1, 2, 3, 4, 5))
    e = ctypes.create_string_buffer(32); emu.emu_adaptor_challenge(e, pts)
    assert int.from_bytes(e.raw, "big") == A.dleq_challenge(*(A.pt_mul(k, A.G) for k in (1, 2, 3, 4, 5)))
    assert len(mid.raw) == 32 and mid.raw != bytes(32)


def test_key_objects_are_the_references(ref):
    """the object layout adaptor_ref.key_object writes is what secp256k1_ec_pubkey_parse of the reference library gives"""
    from tests.tweak_ref import TweakRef
    t = TweakRef()
    for it in A.random_items(8, 5506, corrupt_every=0):
        for key in (it[2], it[4]):
            assert A.key_object(key) == A.key_object(key, t.ec_parse)
    assert A.key_object(b"\x02" + A.b32(A.P)) is None and t.ec_parse(b"\x02" + A.b32(A.P)) is None


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_adaptor" in build_lib.UNITS + build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in ADAPTOR_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name


def test_library_exports_adaptor():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in ADAPTOR_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine / group: the call fails with a message, whatever the device situation
    assert lib.secp256k1_ecdsa_adaptor_verify_batch(None, None, None, None, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_adaptor_verify_batch_dev(None, None, None, None, None, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_adaptor_verify_batch_group(None, None, None, None, None, None, 0, 1) == 0 and "null group" in _native.last_error()
    assert lib.s2k_ecmult2_batch(None, None, None, None, None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.s2k_ecmult2_batch_dev(None, None, None, None, None, None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    # the single-item form: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched
    obj = ctypes.create_string_buffer(b"\x01" * 64, 64)
    for args in ((None, obj, bytes(32), obj), (bytes(162), None, bytes(32), obj), (bytes(162), obj, None, obj), (bytes(162), obj, bytes(32), None)):
        assert lib.secp256k1_ecdsa_adaptor_verify_amd(None, *args) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    g = api.Group.__new__(api.Group)
    for obj in (e, g):
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(162), bytes(33), bytes(32), bytes(33), pk_format=3)
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(162), bytes(33), bytes(32), bytes(33), pk_format=1)      # objects are 64 bytes
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(162), bytes(33), bytes(32), bytes(64))                   # both key arrays share the format
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(161), bytes(33), bytes(32), bytes(33))
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(162), bytes(33), bytes(31), bytes(33))
        with pytest.raises(ValueError):
            obj.ecdsa_adaptor_verify_batch(bytes(162), None, bytes(32), bytes(33))
    with pytest.raises(ValueError):
        e.ecmult2_batch(bytes(64), bytes(32), bytes(64), bytes(31))
    with pytest.raises(ValueError):
        e.ecmult2_batch(bytes(64), bytes(32), bytes(128), bytes(32))
    with pytest.raises(ValueError):
        e.ecmult2_batch(bytes(64), bytes(32), bytes(64), bytes(32), b_inf=bytes(2))
    with pytest.raises(ValueError):
        e.ecmult2_batch(bytes(64), bytes(32), None, bytes(32))


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_ecdsa_adaptor_verify_batch(0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_ecdsa_adaptor_verify_amd(0, 0, 0, 0, 0) + s2k_ecmult2_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "adaptor_verify.c"), "-o", str(tmp_path / "e.o")], check=True)
