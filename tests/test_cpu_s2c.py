"""CPU tier: ECDSA sign-to-contract checks and anti-exfil host verification.  secp256k1_zkp_amd/csrc/s2c.h runs on the host
(tests/host_emul/s2c_emu.cpp, S2K_VERIFY on, 12-bit generator table) against the Python model of tests/s2c_ref.py and the recorded vectors
(tests/golden/s2c_vectors.json: the verdicts of the reference's own secp256k1_ecdsa_s2c_verify_commit and secp256k1_anti_exfil_host_verify);
plus the midstates, the x(R) >= n branch of the comparison, the ABI, the argument checks and the C example."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import s2c_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
S2C_SYMBOLS = ["secp256k1_ecdsa_s2c_verify_commit_batch", "secp256k1_ecdsa_s2c_verify_commit_batch_dev", "secp256k1_ecdsa_s2c_verify_commit_batch_group",
               "secp256k1_anti_exfil_host_verify_batch", "secp256k1_anti_exfil_host_verify_batch_dev", "secp256k1_anti_exfil_host_verify_batch_group",
               "secp256k1_ecdsa_anti_exfil_host_commit_batch", "secp256k1_ecdsa_anti_exfil_host_commit_batch_dev",
               "secp256k1_ecdsa_s2c_verify_commit_amd", "secp256k1_anti_exfil_host_verify_amd"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_s2c_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_s2c_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    cp = ctypes.c_char_p
    lib.emu_s2c_commit.argtypes = [cp, ctypes.c_size_t, ctypes.c_int, cp, cp, ctypes.c_int]
    lib.emu_s2c_host_verify.argtypes = [cp, ctypes.c_size_t, ctypes.c_int, cp, cp, ctypes.c_int, cp, cp, ctypes.c_int]
    lib.emu_s2c_host_commit.argtypes = [cp, cp]
    lib.emu_s2c_tweak.argtypes = [cp, cp, cp, ctypes.c_int]
    lib.emu_s2c_midstates.argtypes = [cp]
    lib.emu_s2c_x_matches.argtypes = [cp, cp, cp]
    return lib


def fixture_file():
    return json.load(open(os.path.join(HERE, "golden", "s2c_vectors.json")))


def golden():
    return S.from_json(fixture_file()["vectors"])


def _run_items(emu, items, combos=S.FORMAT_COMBINATIONS):
    """every item through both host-emulated lane routines, in every format combination it exists in"""
    ran = 0
    for it in items:
        for sf, pf, of in combos:
            got = S.keys_in_format(it, sf, pf, of)
            if got is None:
                continue
            sig, pk, op = got
            if pf == 0:                                   # (the commitment check reads no key: once per signature and opening format)
                assert emu.emu_s2c_commit(sig, len(sig), sf, it[4], op, of) == it[6], (it[0], sf, of)
            assert emu.emu_s2c_host_verify(sig, len(sig), sf, it[2], pk, pf, it[4], op, of) == it[7], (it[0], sf, pf, of)
            ran += 1
    return ran


def test_golden_fixture_shape():
    f = fixture_file()
    v = golden()
    names = {x[0]: x for x in v}
    assert len(names) == len(v) and sum(1 for x in v if x[0].startswith("random ")) == 64
    assert os.path.getsize(os.path.join(HERE, "golden", "s2c_vectors.json")) <= os.path.getsize(os.path.join(HERE, "golden", "adaptor_vectors.json"))
    for i in range(2):
        assert names["module vector %d" % i][6:8] == (1, 1) and names["module vector %d anti-exfil" % i][6:8] == (1, 1)
        assert names["module vector %d with the exfil opening" % i][6:8] == (0, 0)
    assert names["module vector 0"][5].hex().startswith("03f030de") and names["module vector 0"][5].hex().endswith("7d3a")
    assert all(len(x[2]) == 32 and len(x[4]) == 32 for x in v) and all(len(x[1]) == 64 and len(x[3]) == 33 and len(x[5]) == 33 for x in v if x[8] is None)
    assert all(x[7] <= x[6] for x in v)                                                    # host verification implies the commitment check
    assert sorted(x[8] for x in v if x[8] is not None) == ["der"] * 3 + ["obj_opening", "obj_pubkey", "obj_sig", "obj_sig"]
    rnd = [x for x in v if x[0].startswith("random ")]
    assert all(x[6:8] == (1, 1) for i, x in enumerate(rnd) if i % 4 != 3) and all(x[7] == 0 for i, x in enumerate(rnd) if i % 4 == 3)
    assert 0 < sum(x[6] for i, x in enumerate(rnd) if i % 4 == 3) < 16                    # flipped bits of both kinds: (1, 0) and (0, 0)
    assert len(f["host_commit"]) == 10


def test_model_against_fixture():
    """the Python model returns the reference's recorded verdicts on every item the reference was asked, and its recorded host commitments"""
    for name, sig, msg, pk, data, op, c, h, only in golden():
        if only is None:
            assert (S.verify_commit(sig, data, op), S.host_verify(sig, msg, pk, data, op)) == (c, h), name
        elif only == "der":
            rs = S.parse_der(sig)
            cc = S.commit_rs(rs, data, S.parse33(op))
            assert (cc, cc & S.ecdsa_rs(rs, msg, S.parse33(pk))) == (c, h), name
    for rnd, cm in fixture_file()["host_commit"]:
        assert S.host_commit(bytes.fromhex(rnd)).hex() == cm


def test_edge_list_verdicts():
    """the edge list rebuilt now is the recorded one, and each item has the verdicts its name promises"""
    cases = S.edge_cases()
    assert cases == [x for x in golden() if not x[0].startswith(("random ", "module "))]
    for it in cases:
        assert it[6:8] == S.EDGE_VERDICTS.get(it[0], (0, 0)), it[0]
    names = {x[0] for x in cases}
    assert set(S.EDGE_VERDICTS) <= names and len(names) == len(cases)
    for need in ("valid", "one data bit flipped", "opening negated", "opening of another item", "opening with prefix 04", "opening with prefix 00",
                 "opening with x >= p", "opening with x not on the curve", "all-zero opening object", "r + 1", "r = 0", "r >= n in compact form",
                 "s >= n in compact form", "object limbs >= n: r", "object limbs >= n: s", "s -> n - s", "s = 0", "message + 1", "public key negated",
                 "public key unparsable", "all-zero public-key object", "valid plain ECDSA signature with an unrelated opening", "valid DER signature",
                 "DER signature with a trailing byte"):
        assert need in names, need
    # the plain signature is a valid ECDSA signature: only the commitment half refuses the item
    it = next(x for x in cases if x[0].startswith("valid plain ECDSA"))
    assert S.ecdsa_rs(S.parse_compact(it[1]), it[2], S.parse33(it[3])) == 1


def test_model_signer_and_parsers():
    rng = np.random.default_rng(5603)
    for _ in range(4):
        d, k = S._rand_scalar(rng), S._rand_scalar(rng)
        msg, data = S._rand32(rng), S._rand32(rng)
        sig, op = S.sign(d, msg, k, data)
        pk = S.ser33(S.pt_mul(d, S.G))
        assert S.host_verify(sig, msg, pk, data, op) == 1 and S.verify_commit(sig, S._flip(data, 3), op) == 0
        rs = S.parse_compact(sig)
        assert S.parse_der(S.der_encode(*rs)) == rs and S.parse_der(S.der_encode(*rs) + b"\0") is None and S.parse_der(S.der_encode(*rs)[:-1]) is None
    assert S.parse_der(S.der_encode(S.N, 1)) == (0, 1) and S.parse_der(b"") is None and S.parse_der(b"\x30\x80") is None


def test_emu_golden(emu):
    """the recorded vectors in every format combination they exist in (no reference needed)"""
    assert _run_items(emu, golden()) >= 18 * 60


def test_emu_random_against_model(emu):
    """256 seeded items, one in four corrupted, in every format an item exists in"""
    items = S.random_items(256, 5604)
    commit, host = sum(x[6] for x in items), sum(x[7] for x in items)
    assert host == 192 and 192 < commit < 256
    assert _run_items(emu, items) >= 18 * 240


def test_emu_tweak_and_host_commit_against_hashlib(emu):
    """the two-block hash put together from words is SHA-256 of tag | tag | ser33(opening) | data, in both opening formats; the one-block
    hash is SHA-256 of tag | tag | rand"""
    rng = np.random.default_rng(5606)
    tp, td = hashlib.sha256(S.TAG_POINT).digest(), hashlib.sha256(S.TAG_DATA).digest()
    for i in range(16):
        O = S.pt_mul(S._rand_scalar(rng), S.G)
        data = S._rand32(rng) if i else b"\xff" * 32
        want = hashlib.sha256(tp + tp + S.ser33(O) + data).digest()
        for fmt, op in ((0, S.ser33(O)), (1, S.key_object(S.ser33(O)))):
            t = ctypes.create_string_buffer(32)
            assert emu.emu_s2c_tweak(t, data, op, fmt) == 1 and t.raw == want, (i, fmt)
        out = ctypes.create_string_buffer(32); emu.emu_s2c_host_commit(out, data)
        assert out.raw == hashlib.sha256(td + td + data).digest()
    for rnd, cm in fixture_file()["host_commit"]:
        out = ctypes.create_string_buffer(32); emu.emu_s2c_host_commit(out, bytes.fromhex(rnd))
        assert out.raw.hex() == cm


def test_midstates_against_a_compression_from_the_initial_state(emu):
    """both midstates the engine derives are the SHA-256 state after one compression of SHA256(tag) | SHA256(tag) from the initial state
    (tests/s2c_ref.py: sha256_compress, itself checked against hashlib here)"""
    block = bytes(range(55)) + b"\x80" + (55 * 8).to_bytes(8, "big")
    assert b"".join(w.to_bytes(4, "big") for w in S.sha256_compress(S.SHA_IV, block)) == hashlib.sha256(bytes(range(55))).digest()
    mid = ctypes.create_string_buffer(64); emu.emu_s2c_midstates(mid)
    want = b"".join(w.to_bytes(4, "big") for tag in (S.TAG_POINT, S.TAG_DATA) for w in S.tag_midstate(tag))
    assert mid.raw == want and mid.raw[:32] != mid.raw[32:]


def test_x_above_n_primitive(emu):
    """s2c_x_matches where no entry point takes it: x(R) = n + k with r = k (the second branch) and r = k + 1, small x in the first branch"""
    cases = S.x_above_n_cases()
    assert sum(1 for c in cases if c[0].startswith("x = n + ") and c[4] == 1) == 4 and sum(c[4] for c in cases) == 12 and len(cases) == 28
    for name, xy, z, r, want in cases:
        x = int.from_bytes(xy[:32], "big")
        assert (x % S.N == int.from_bytes(r, "big")) == bool(want), name                  # the expected value is x mod n == r
        assert emu.emu_s2c_x_matches(xy, z, r) == want, name


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_s2c" in build_lib.UNITS_ADDED and build_lib.UNITS_ADDED.index("engine_s2c") < build_lib.UNITS_ADDED.index("engine_musig_agg")
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in S2C_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "src/modules/ecdsa_s2c/main_impl.h:88" in hdr and "src/modules/ecdsa_s2c/main_impl.h:185" in hdr
    from secp256k1_zkp_amd import api
    assert "#define S2K_OPT_S2C_FUSED 13" in hdr and api.Engine.OPT_S2C_FUSED == 13


def test_library_exports_s2c():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in S2C_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine / group: the call fails with a message, whatever the device situation
    assert lib.secp256k1_ecdsa_s2c_verify_commit_batch(None, None, None, None, 0, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_s2c_verify_commit_batch_dev(None, None, None, None, None, 0, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_anti_exfil_host_verify_batch(None, None, None, None, 0, None, None, 0, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_anti_exfil_host_verify_batch_dev(None, None, None, None, None, 0, None, None, 0, None, None, 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_anti_exfil_host_commit_batch(None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_s2c_verify_commit_batch_group(None, None, None, None, 0, None, None, 0, 1) == 0 and "null group" in _native.last_error()
    assert lib.secp256k1_anti_exfil_host_verify_batch_group(None, None, None, None, 0, None, None, 0, None, None, 0, 1) == 0 and "null group" in _native.last_error()
    # the single-item forms: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched
    obj = ctypes.create_string_buffer(b"\x01" * 64, 64)
    for args in ((None, bytes(32), obj), (obj, None, obj), (obj, bytes(32), None)):
        assert lib.secp256k1_ecdsa_s2c_verify_commit_amd(None, *args) == 0 and lib.s2k_last_status() == 2
    good = [obj, bytes(32), obj, bytes(32), obj]
    for k in range(5):
        a = list(good); a[k] = None
        assert lib.secp256k1_anti_exfil_host_verify_amd(None, *a) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    g = api.Group.__new__(api.Group)
    for obj in (e, g):
        for bad in (dict(opening_format=2), dict(opening_format=1), dict(sig_format=3)):
            with pytest.raises(ValueError):
                obj.ecdsa_s2c_verify_commit_batch(bytes(64), bytes(32), bytes(33), **bad)
        with pytest.raises(ValueError):
            obj.ecdsa_s2c_verify_commit_batch(bytes(63), bytes(32), bytes(33))
        with pytest.raises(ValueError):
            obj.ecdsa_s2c_verify_commit_batch(bytes(64), bytes(31), bytes(33))
        with pytest.raises(ValueError):
            obj.ecdsa_s2c_verify_commit_batch(bytes(64), bytes(32), None)
        for bad in (dict(opening_format=2), dict(pk_format=3), dict(pk_format=1), dict(opening_format=1)):
            with pytest.raises(ValueError):
                obj.anti_exfil_host_verify_batch(bytes(64), bytes(32), bytes(33), bytes(32), bytes(33), **bad)
        with pytest.raises(ValueError):
            obj.anti_exfil_host_verify_batch(bytes(64), bytes(32), bytes(33), bytes(31), bytes(33))
        with pytest.raises(ValueError):
            obj.anti_exfil_host_verify_batch(bytes(64), bytes(32), None, bytes(32), bytes(33))
        with pytest.raises(ValueError):
            obj.anti_exfil_host_verify_batch(bytes(64), bytes(32), bytes(33), bytes(32), bytes(34))
    with pytest.raises(ValueError):
        e.anti_exfil_host_commit_batch(bytes(33))
    with pytest.raises(ValueError):
        e.anti_exfil_host_commit_batch(None)


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_ecdsa_s2c_verify_commit_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_anti_exfil_host_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_ecdsa_anti_exfil_host_commit_batch(0, 0, 0, 0) + '
                   'secp256k1_ecdsa_s2c_verify_commit_amd(0, 0, 0, 0) + secp256k1_anti_exfil_host_verify_amd(0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "anti_exfil_verify.c"), "-o", str(tmp_path / "e.o")], check=True)
