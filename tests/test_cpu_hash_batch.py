"""CPU tier: batch SHA-256, tagged hashes and BIP-340 with a message length per item.  secp256k1_zkp_amd/csrc/hash_batch.h runs on the
host (tests/host_emul/hash_batch_emu.cpp) against hashlib and the unmodified reference (oracle/_ref through tests/hash_ref.py); the
stand-alone tests/host_emul/hash_batch_bounds runs it under the sanitizers with every message in an allocation of exactly its length;
plus the ABI, the argument checks that run in front of any device, the build entry and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import hash_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HASH_SYMBOLS = ["s2k_sha256_batch", "s2k_sha256_batch_dev", "secp256k1_tagged_sha256_batch", "secp256k1_tagged_sha256_batch_dev", "secp256k1_tagged_sha256_amd",
                "secp256k1_schnorrsig_verify_batch_var", "secp256k1_schnorrsig_verify_batch_var_dev"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_hash_batch_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_hash_batch_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.emu_hash_batch.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, vp, vp, ctypes.c_size_t, ctypes.c_size_t]
    lib.emu_schnorr_verify_var.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_size_t]
    return lib


@pytest.fixture(scope="module")
def href(ref):
    return H.HashRef()


def _emu_digests(emu, mode, tag, buf, off=None, msglen=0, n=None):
    """buf: an exact-size numpy array; -> n digests as bytes"""
    n = off.size - 1 if off is not None else n
    out = np.full((n, 32), 0xEE, np.uint8)
    assert emu.emu_hash_batch(out.ctypes.data, mode, tag, len(tag), buf.ctypes.data, off.ctypes.data if off is not None else None, msglen, n) == 1
    return [out[i].tobytes() for i in range(n)]


MODES = [(0, b"")] + [(1, b"")] + [(2, t) for t in H.TAGS]


def test_emu_every_length_at_every_offset(emu):
    """lengths 0 .. 300 back to back, the first item starting 0 .. 15 bytes into the buffer: every alignment of every length's word loads"""
    rng = np.random.default_rng(3402)
    msgs = [H.message(rng, ln) for ln in range(301)]
    want = {m: [H.digest(m[0], m[1], x) for x in msgs] for m in MODES}
    blob, off = H.pack(msgs)
    for k in range(16):
        buf = np.concatenate([np.full(k, 0xA5, np.uint8), blob])                # ends with the last item
        o = off + np.uint64(k)
        for m in MODES:
            assert _emu_digests(emu, m[0], m[1], buf, o) == want[m], (k, m)


def test_emu_fixed_length_form(emu):
    rng = np.random.default_rng(3403)
    for ln in H.FIXED_LENGTHS:
        msgs = [H.message(rng, ln) for _ in range(5)]
        buf = np.frombuffer(b"".join(msgs) or b"\x00", np.uint8).copy()
        for m in MODES[:3]:
            assert _emu_digests(emu, m[0], m[1], buf, None, ln, 5) == [H.digest(m[0], m[1], x) for x in msgs], (ln, m)


def test_emu_long_message(emu):
    """2^20 + 3 bytes: 16 384 full blocks, then a three-byte tail"""
    rng = np.random.default_rng(3404)
    buf = rng.integers(0, 256, (1 << 20) + 3, dtype=np.uint8)
    off = np.array([0, buf.size], np.uint64)
    for m in MODES[:3]:
        assert _emu_digests(emu, m[0], m[1], buf, off) == [H.digest(m[0], m[1], buf.tobytes())], m


def test_emu_decreasing_offsets_give_zero_bytes(emu):
    """the rule of the _dev forms: such an item is 32 zero bytes, never the digest of the empty message; its neighbours are right"""
    buf = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 5, 40, 40], np.uint64)
    for m in MODES[:3]:
        got = _emu_digests(emu, m[0], m[1], buf, off)
        b = buf.tobytes()
        assert got == [H.digest(m[0], m[1], b[0:10]), bytes(32), H.digest(m[0], m[1], b[5:40]), H.digest(m[0], m[1], b"")], m


def test_emu_tagged_against_reference(emu, href):
    rng = np.random.default_rng(3405)
    for tag in H.TAGS:
        msgs = [H.message(rng, ln) for ln in (0, 1, 31, 32, 33, 64, 100)]
        blob, off = H.pack(msgs)
        want = [href.tagged_sha256(tag, x) for x in msgs]
        assert want == [H.tagged(tag, x) for x in msgs]
        assert _emu_digests(emu, 2, tag, blob, off) == want, tag


def test_bounds_program():
    """every message of 0 .. 200 bytes in a heap allocation of exactly its length, address and undefined-behaviour sanitizers on: exit status 0
    shows that no byte outside an item is read (stand-alone program: nothing is preloaded)"""
    exe = os.path.join(HERE, "host_emul", "hash_batch_bounds")
    assert os.path.exists(exe), "tests/host_emul/hash_batch_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 603", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _emu_var(emu, b, pk_format):
    n = b["sigs"].shape[0]
    res = np.full(n, 7, np.int32)
    pk = b["pkobj"] if pk_format else b["pk32"]
    blob = b["blob"] if b["blob"].size else np.zeros(1, np.uint8)
    assert emu.emu_schnorr_verify_var(res.ctypes.data, b["sigs"].ctypes.data, blob.ctypes.data, b["off"].ctypes.data, pk.ctypes.data, pk_format, n) == 1
    return res


def test_emu_schnorr_var_against_reference(emu, href):
    b = href.var_cases()
    n = b["expected"].size
    ones = int(b["expected"].sum())
    assert 3 * ones >= n and 3 * (n - ones) >= n, (ones, n)
    for name, v in zip(b["names"], b["expected"]):
        assert v == (1 if "valid" in name else 0), name                           # what the list is built to be
    for pk_format in (0, 1):
        got = _emu_var(emu, b, pk_format)
        assert got.tolist() == b["expected"].tolist(), [nm for nm, g, w in zip(b["names"], got, b["expected"]) if g != w]
    # a decreasing pair (the _dev rule): verdict 0 for that item, the others as before
    off = b["off"].copy()
    b2 = dict(b, off=off)
    off[1] = off[0] + 5000                                                       # item 0 ends behind where item 1 ends: item 1's pair decreases
    got = _emu_var(emu, dict(b2, blob=np.concatenate([b["blob"], np.zeros(5000, np.uint8)])), 0)
    assert got[1] == 0 and got[0] == 0 and got[2:].tolist() == b["expected"][2:].tolist()


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, api, build_lib
    units = build_lib.UNITS + build_lib.UNITS_ADDED
    assert len(build_lib.UNITS) == 7 and units[-2:] == ["engine_schnorr_all", "engine_musig_agg"]
    assert units.index("engine_pubkey") < units.index("engine_hash") < units.index("engine_schnorr_all")
    for f in ("engine_hash.hip", "hash_batch.h"):
        assert os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", f)), f
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in HASH_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    for m in ("sha256_batch", "tagged_sha256_batch", "schnorrsig_verify_batch_var"):
        assert callable(getattr(api.Engine, m)) and callable(getattr(api.Engine, m + "_dev")), m
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "hash_batch_emu.cpp" in entry and "libs2k_hash_batch_emu.so" in entry and '"hash_batch_bounds"' in entry


def test_documents_name_the_calls():
    for doc in ("README.md", "DESIGN.md", "SURVEY.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ("s2k_sha256_batch", "secp256k1_tagged_sha256_batch", "secp256k1_schnorrsig_verify_batch_var"):
            assert name in text, (doc, name)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "engine_hash.hip" in readme and "7.11" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_library_exports_hash():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in HASH_SYMBOLS:
        assert hasattr(lib, name) and (" T " + name + "\n") in out, name
    o = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert lib.s2k_sha256_batch(None, o, bytes(8), None, 8, 1, 1) == 0 and "null engine" in _native.last_error()
    assert lib.s2k_sha256_batch_dev(None, None, o, bytes(8), None, 8, 1, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_tagged_sha256_batch(None, o, b"t", 1, bytes(8), None, 8, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_tagged_sha256_batch_dev(None, None, o, b"t", 1, bytes(8), None, 8, 1) == 0 and "null engine" in _native.last_error()
    off = np.array([0, 8], np.uint64)
    assert lib.secp256k1_schnorrsig_verify_batch_var(None, o, bytes(64), bytes(8), off.ctypes.data, bytes(32), 0, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_schnorrsig_verify_batch_var_dev(None, None, o, bytes(64), bytes(8), off.ctypes.data, bytes(32), 0, 1) == 0 and "null engine" in _native.last_error()
    assert o.raw == b"\xff" * 32


def test_single_item_form_checks_its_arguments_first():
    """NULL where the reference has ARG_CHECK is an illegal argument before any device is touched; nothing is written"""
    from secp256k1_zkp_amd import _native
    lib = _native.load()
    S = lib.s2k_last_status
    o = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert lib.secp256k1_tagged_sha256_amd(None, None, b"tag", 3, b"msg", 3) == 0 and S() == 2
    assert lib.secp256k1_tagged_sha256_amd(None, o, None, 3, b"msg", 3) == 0 and S() == 2 and o.raw == b"\xff" * 32
    assert lib.secp256k1_tagged_sha256_amd(None, o, b"tag", 3, None, 3) == 0 and S() == 2 and o.raw == b"\xff" * 32
    assert lib.secp256k1_tagged_sha256_amd(None, o, b"tag", 3, None, 0) == 0 and S() == 2 and o.raw == b"\xff" * 32      # (the reference checks msg != NULL whatever msglen is)


def test_python_argument_checks():
    """run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    for call in (lambda **kw: e.sha256_batch(bytes(64), **kw), lambda **kw: e.tagged_sha256_batch(b"t", bytes(64), **kw)):
        with pytest.raises(ValueError):
            call()                                                                # neither
        with pytest.raises(ValueError):
            call(msg_off=[0, 64], msglen=64)                                      # both
        with pytest.raises(api.S2KError):
            call(msg_off=[])
        with pytest.raises(ValueError):
            call(msg_off=[0, 65])                                                 # behind the data
        with pytest.raises(ValueError):
            call(msglen=48)                                                       # 64 bytes are not n * 48
        with pytest.raises(ValueError):
            call(msglen=0)                                                        # n unknown
    with pytest.raises(ValueError):
        e.sha256_batch(None, msglen=1)
    with pytest.raises(ValueError):
        e.tagged_sha256_batch(None, bytes(4), msglen=4)
    with pytest.raises(api.S2KError):
        e.schnorrsig_verify_batch_var(bytes(64), bytes(8), [], bytes(32))
    for args, kw in (((bytes(64), bytes(8), None, bytes(32)), {}), ((bytes(63), bytes(8), [0, 8], bytes(32)), {}), ((bytes(64), bytes(8), [0, 8], bytes(64)), {}),
                     ((bytes(64), bytes(8), [0, 9], bytes(32)), {}), ((bytes(64), bytes(8), [0, 8], bytes(32)), dict(pk_format=2))):
        with pytest.raises(ValueError):
            e.schnorrsig_verify_batch_var(*args, **kw)
    with pytest.raises(ValueError):
        e.sha256_batch_dev(None, None)
    with pytest.raises(ValueError):
        e.schnorrsig_verify_batch_var_dev(None, None, None, None, None)


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return s2k_sha256_batch(0, 0, 0, 0, 0, 2, 0) + s2k_sha256_batch_dev(0, 0, 0, 0, 0, 0, 1, 0) + '
                   'secp256k1_tagged_sha256_batch(0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_tagged_sha256_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_tagged_sha256_amd(0, 0, 0, 0, 0, 0) + secp256k1_schnorrsig_verify_batch_var(0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_schnorrsig_verify_batch_var_dev(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "sha256_batch.c"), "-o", str(tmp_path / "e.o")], check=True)
