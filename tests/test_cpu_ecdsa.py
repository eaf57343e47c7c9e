"""CPU tier: ECDSA verification and recovery.  secp256k1_zkp_amd/csrc/ecdsa.h runs on the host (tests/host_emul/ecdsa_emu.cpp, S2K_VERIFY on)
against the unmodified reference (oracle/_ref through tests/ecdsa_ref.py): the Wycheproof set, random signatures in every encoding, the edge
list; plus the ABI, the Python argument checks and the C example."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PK_BYTES = {0: 33, 1: 64, 2: 65}


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ecdsa_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ecdsa_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_ecdsa_verify.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    lib.emu_ecdsa_recover.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p]
    lib.emu_ecdsa_sig_load.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.emu_ecdsa_pubkey_load.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def eref(ref):
    from tests.ecdsa_ref import EcdsaRef
    return EcdsaRef()


def wycheproof():
    g = json.load(open(os.path.join(HERE, "golden", "ecdsa_wycheproof.json")))
    keys = [bytes.fromhex(k) for k in g["keys"]]
    return [(tc, keys[k], bytes.fromhex(h), bytes.fromhex(sig), verdict) for tc, k, h, sig, verdict in g["vectors"]]


def _verify(emu, sig, sf, msg, pk, pf):
    sig = bytes(sig)
    return emu.emu_ecdsa_verify(sig, len(sig), sf, bytes(msg), bytes(pk), pf)


def test_wycheproof_fixture_shape():
    v = wycheproof()
    assert len(v) == 463 and sum(x[4] for x in v) == 162 and len({x[1] for x in v}) == 99
    assert max(len(x[3]) for x in v) == 4172


def test_emu_wycheproof(emu):
    """all 463 vectors in DER form, verdict by verdict (the fixture's verdicts were recomputed with the reference when it was written)"""
    for tc, key, h, sig, verdict in wycheproof():
        assert _verify(emu, sig, 2, h, key, 2) == verdict, tc


def test_emu_wycheproof_against_reference(emu, eref):
    """the same with the reference asked now, and the DER parser on its own: accepted / refused and the integers it yields"""
    for tc, key, h, sig, verdict in wycheproof():
        assert eref.verify(sig, 2, h, key, 2) == verdict, tc
        so = eref.sig_parse_der(sig)
        rs = ctypes.create_string_buffer(64)
        assert emu.emu_ecdsa_sig_load(rs, sig, len(sig), 2) == (so is not None), tc
        if so is not None:
            assert rs.raw == eref.sig_serialize_compact(so), tc


def test_emu_der_parser_shapes(emu, eref):
    from tests.ecdsa_ref import edge_cases
    rng = np.random.default_rng(11)
    cases = edge_cases(eref, rng)
    ders = [c[1] for c in cases if c[2] == 2]
    # single-byte mutations and truncations of a valid encoding: every decision of the length and integer readers
    base = [c[1] for c in cases if c[0] == "DER valid"][0]
    for i in range(len(base)):
        for v in (0x00, 0x01, 0x7F, 0x80, 0x81, 0xFF, base[i] ^ 0x80):
            ders.append(base[:i] + bytes([v]) + base[i + 1:])
        ders.append(base[:i])
    assert len(ders) > 500 and len(base) >= 70
    accepted = 0
    for d in ders:
        so = eref.sig_parse_der(d)
        rs = ctypes.create_string_buffer(64)
        assert emu.emu_ecdsa_sig_load(rs, d, len(d), 2) == (so is not None), d.hex()
        if so is not None:
            accepted += 1
            assert rs.raw == eref.sig_serialize_compact(so), d.hex()
    assert accepted > 50


@pytest.mark.parametrize("sig_format", [0, 1, 2])
@pytest.mark.parametrize("pk_format", [0, 1, 2])
def test_emu_random(emu, eref, sig_format, pk_format):
    """512 random signatures per encoding pair, 1/8 of them corrupted in r, s, message or key"""
    from tests.ecdsa_ref import corrupt
    rng = np.random.default_rng(100 + 3 * sig_format + pk_format)
    n = 512
    d = eref.make(n, rng)
    msgs = d["msgs"].copy()
    pks = eref.pks_as(d["pkobj"], pk_format)
    s64 = eref.sigs_as(d["sigobj"], 0 if sig_format == 2 else sig_format)          # corrupt r and s where they are plain bytes ...
    idx = corrupt(rng, s64, msgs, pks, 1 / 8)
    assert 40 <= len(idx) <= 90
    if sig_format == 2:                                                            # ... and DER-encode what came out
        from tests.ecdsa_ref import der_encode
        sigs = [der_encode(int.from_bytes(s64[i, :32].tobytes(), "big"), int.from_bytes(s64[i, 32:].tobytes(), "big")) for i in range(n)]
    else:
        sigs = s64
    exp = eref.verify_many(sigs, sig_format, msgs, pks, pk_format)
    got = np.array([_verify(emu, bytes(sigs[i]) if sig_format == 2 else sigs[i].tobytes(), sig_format, msgs[i].tobytes(), pks[i].tobytes(), pk_format) for i in range(n)], np.int32)
    assert (got == exp).all(), np.flatnonzero(got != exp)
    ok = np.ones(n, bool); ok[idx] = False
    assert exp[ok].all() and exp.sum() >= n - len(idx)
    if pk_format != 1:                     # (a corrupted key OBJECT is a different valid-looking point: no curve check, as the reference)
        assert exp.sum() < n - len(idx) // 2


def test_emu_edges(emu, eref):
    from tests.ecdsa_ref import edge_cases
    cases = edge_cases(eref, np.random.default_rng(12))
    assert len(cases) >= 70 and 10 <= sum(c[-1] for c in cases) < len(cases)
    for name, sig, sf, msg, pk, pf, expected in cases:
        assert _verify(emu, sig, sf, msg, pk, pf) == expected, name


def test_emu_pubkey_parsers(emu, eref):
    """the three key encodings give the same point as the reference's parser (read back from its 64-byte object)"""
    rng = np.random.default_rng(13)
    d = eref.make(32, rng)
    for i in range(32):
        obj = d["pkobj"][i].tobytes()
        want = obj[:32][::-1] + obj[32:][::-1]
        for pf in (0, 1, 2):
            ser = eref.pks_as(d["pkobj"][i:i + 1], pf)[0].tobytes()
            xy = ctypes.create_string_buffer(64)
            assert emu.emu_ecdsa_pubkey_load(xy, ser, pf) == 1 and xy.raw == want
        hyb = bytes([6 + (want[63] & 1)]) + want
        assert emu.emu_ecdsa_pubkey_load(xy, hyb, 2) == 1 and eref.pubkey_parse(hyb) == obj


def test_emu_recover(emu, eref):
    """256 reference-made recoverable signatures: the key object byte for byte; each with the three other recids; the edge list"""
    from tests.ecdsa_ref import recover_cases
    rng = np.random.default_rng(14)
    n = 256
    msgs, sigs, recids, pkobj = eref.make_recoverable(n, rng)
    assert set(recids.tolist()) <= {0, 1, 2, 3} and len(set(recids.tolist())) >= 2
    out = ctypes.create_string_buffer(64)
    for i in range(n):
        s, m = sigs[i].tobytes(), msgs[i].tobytes()
        assert emu.emu_ecdsa_recover(out, s, int(recids[i]), m) == 1
        assert out.raw == pkobj[i].tobytes(), i
        assert _verify(emu, s, 0, m, out.raw, 1) == 1
        for k in range(4):
            if k == recids[i]:
                continue
            v, pk = eref.recover(s, k, m)
            assert emu.emu_ecdsa_recover(out, s, k, m) == v and out.raw == pk, (i, k)
    cases = recover_cases(eref, np.random.default_rng(15))
    assert sum(c[4] for c in cases) >= 10
    for name, sig, recid, msg, v, pk in cases:
        out = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert emu.emu_ecdsa_recover(out, sig, recid, msg) == v, name
        assert out.raw == pk, name
    names = [c[0] for c in cases]
    assert "recid 4" in names and "recid 255" in names


# ---- ABI, Python layer, C example ----------------------------------------------------------------------------------------------------
ECDSA_SYMBOLS = ["secp256k1_ecdsa_verify_batch", "secp256k1_ecdsa_verify_batch_dev", "secp256k1_ecdsa_verify_batch_group", "secp256k1_ecdsa_recover_batch",
                 "secp256k1_ecdsa_recover_batch_dev", "secp256k1_ecdsa_verify_amd", "secp256k1_ecdsa_recover_amd"]


def test_abi_has_ecdsa():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_ecdsa" in build_lib.UNITS and len(build_lib.UNITS) == 7
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in ECDSA_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name


def test_library_exports_ecdsa():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in ECDSA_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine: the call fails with a message, whatever the device situation
    assert lib.secp256k1_ecdsa_verify_batch(None, None, None, None, 0, None, None, 0, 1) == 0
    assert "null engine" in _native.last_error()
    assert lib.secp256k1_ecdsa_recover_batch(None, None, None, None, None, None, 1) == 0
    assert lib.secp256k1_ecdsa_verify_amd(None, None, None, None) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_ecdsa_recover_amd(None, None, None, None) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine); g = api.Group.__new__(api.Group)
    for obj in (e, g):
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch(np.zeros(128, np.uint8), np.zeros(64, np.uint8), np.zeros(65, np.uint8))           # 2 sigs, 33 * 2 key bytes wanted
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch(np.zeros(128, np.uint8), np.zeros(32, np.uint8), np.zeros(66, np.uint8))
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch(np.zeros(100, np.uint8), np.zeros(32, np.uint8), np.zeros(33, np.uint8))
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch([b"\x30\x00"], np.zeros(32, np.uint8), np.zeros(64, np.uint8), sig_format=2, pk_format=2)
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch(np.zeros(64, np.uint8), np.zeros(32, np.uint8), np.zeros(33, np.uint8), sig_format=3)
        with pytest.raises(ValueError):
            obj.ecdsa_verify_batch((np.zeros(8, np.uint8), np.array([0, 9], np.uint64)), np.zeros(32, np.uint8), np.zeros(33, np.uint8), sig_format=2)
    with pytest.raises(ValueError):
        e.ecdsa_recover_batch(np.zeros(128, np.uint8), np.zeros(1, np.uint8), np.zeros(64, np.uint8))
    data, off = api.Engine.pack([b"\x30\x00", b"", b"\x01\x02\x03"])
    assert off.tolist() == [0, 2, 2, 5] and data.tobytes() == b"\x30\x00\x01\x02\x03"


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_ecdsa_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_ecdsa_recover_amd(0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "ecdsa_verify.c"), "-o", str(tmp_path / "e.o")], check=True)
