"""CPU tier: whitelist-signature verification.  secp256k1_zkp_amd/csrc/whitelist.h runs on the host (tests/host_emul/whitelist_emu.cpp,
S2K_VERIFY on) against the unmodified reference (oracle/_ref through tests/whitelist_ref.py) and the recorded vectors
(tests/golden/whitelist_vectors.json); plus the ABI, the Python argument checks and the C example."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WHITELIST_SYMBOLS = ["secp256k1_whitelist_verify_batch", "secp256k1_whitelist_verify_batch_dev", "secp256k1_whitelist_verify_amd"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_whitelist_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_whitelist_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_whitelist_verify.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.emu_whitelist_key.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def wref(ref):
    from tests.whitelist_ref import WhitelistRef
    return WhitelistRef()


def golden():
    g = json.load(open(os.path.join(HERE, "golden", "whitelist_vectors.json")))
    return [(n, bytes.fromhex(s), bytes.fromhex(on), bytes.fromhex(off), bytes.fromhex(sub), v) for n, s, on, off, sub, v in g["vectors"]]


def _verify(emu, sig, online, offline, sub):
    assert len(online) == len(offline) and len(online) % 64 == 0
    return emu.emu_whitelist_verify(bytes(sig) + b"\0", len(sig), bytes(online) + b"\0", bytes(offline) + b"\0", len(online) // 64, bytes(sub))


def _xy(obj64):
    """secp256k1_pubkey object -> x | y big-endian"""
    return obj64[31::-1] + obj64[:31:-1]


def test_golden_fixture_shape():
    v = golden()
    assert len(v) == 40 and sum(x[5] for x in v) == 13
    assert {len(x[2]) // 64 for x in v} == {0, 1, 2, 3, 15}
    names = {x[0]: x[5] for x in v}
    assert names["crafted n=0"] == 1 and names["offline = -sub"] == 1 and names["offline = sub"] == 1 and names["online = -t (offline + sub)"] == 0


def test_emu_golden(emu):
    """the recorded vectors, verdict by verdict (no reference needed)"""
    for name, sig, on, off, sub, verdict in golden():
        assert _verify(emu, sig, on, off, sub) == verdict, name


def test_emu_edge_list_against_reference(emu, wref):
    """the edge list rebuilt now, the one 255-key signature included; the recorded verdicts are the reference's of today"""
    from tests.whitelist_ref import edge_cases
    cases = edge_cases(wref, with_255=True)
    rec = {x[0]: x for x in golden()}
    for name, sig, on, off, sub, verdict in cases:
        assert _verify(emu, sig, on, off, sub) == verdict, name
        if name in rec:
            assert rec[name][1:] == (sig, on, off, sub, verdict), name
    assert {c[0] for c in cases} - set(rec) == {"valid n=255 signer=100", "n=255 last s flipped"}


def test_emu_random_against_reference(emu, wref):
    """64 seeded items of mixed list lengths 1..8, every fourth one corrupted"""
    from tests.whitelist_ref import random_items
    items = random_items(wref, 64, 3302)
    assert 40 <= sum(x[4] for x in items) <= 48
    for k, (sig, on, off, sub, verdict) in enumerate(items):
        assert _verify(emu, sig, on, off, sub) == verdict, k


def test_emu_ring_key_against_reference(emu, wref):
    """K = online + t (offline + sub) of single pairs against the reference's combine / tweak_mul / combine"""
    from tests.whitelist_ref import Whitelist, ring_key
    rng = np.random.default_rng(3303)
    w = Whitelist(wref, rng, 6)
    sub = wref.pubkey_create(bytes(31) + b"\x07")
    pairs = [(w.online[j], w.offline[j], sub) for j in range(6)]
    pairs.append((w.online[0], wref.pubkey_negate(sub), sub))                        # offline + sub = infinity: K = online
    pairs.append((w.online[1], sub, sub))                                            # a doubling
    a = wref.pubkey_combine([w.offline[2], sub])
    import hashlib
    pairs.append((wref.pubkey_negate(wref.pubkey_tweak_mul(a, hashlib.sha256(wref.pubkey_serialize(a)).digest())), w.offline[2], sub))   # K = infinity
    for k, (on, off, s) in enumerate(pairs):
        xy = ctypes.create_string_buffer(64); inf = ctypes.c_int(-1)
        assert emu.emu_whitelist_key(xy, ctypes.byref(inf), on, off, s) == 1, k
        want = ring_key(wref, on, off, s)
        if want is None:
            assert inf.value == 1 and k == 8
        else:
            assert inf.value == 0 and xy.raw == _xy(want), k
    assert ring_key(wref, *pairs[6]) == w.online[0]
    # a key object that does not load: an infinity record, return 0
    xy = ctypes.create_string_buffer(64); inf = ctypes.c_int(-1)
    assert emu.emu_whitelist_key(xy, ctypes.byref(inf), bytes(64), w.offline[0], sub) == 0 and inf.value == 1


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_whitelist" in build_lib.UNITS + build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in WHITELIST_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name


def test_library_exports_whitelist():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in WHITELIST_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine: the call fails with a message, whatever the device situation
    assert lib.secp256k1_whitelist_verify_batch(None, None, None, None, None, None, None, 0, None, None, 1) == 0
    assert "null engine" in _native.last_error()
    assert lib.secp256k1_whitelist_verify_batch_dev(None, None, None, None, None, None, None, None, 0, None, None, 1) == 0
    assert lib.secp256k1_whitelist_verify_amd(None, None, None, None, 0, None) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    sig = bytes(97); key = bytes(64)
    with pytest.raises(ValueError):
        e.whitelist_verify_batch([sig], [key * 2], [key * 2], bytes(63))                                  # sub: 64 bytes per item
    with pytest.raises(ValueError):
        e.whitelist_verify_batch([sig], [key * 2], [key * 3], bytes(64))                                  # lists of different lengths
    with pytest.raises(ValueError):
        e.whitelist_verify_batch([sig, sig], [key * 2], [key * 2], bytes(128))                            # one list, two items, no list_of
    with pytest.raises(ValueError):
        e.whitelist_verify_batch([sig, sig], [key * 2], [key * 2], bytes(128), list_of=[0])               # list_of: one entry per item
    with pytest.raises(ValueError):
        e.whitelist_verify_batch([sig], key * 2, key * 2, bytes(64), list_off=[0, 3])                     # list_off runs past the keys
    with pytest.raises(ValueError):
        e.whitelist_verify_batch((np.zeros(8, np.uint8), np.array([0, 9], np.uint64)), [key], [key], bytes(64))


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_whitelist_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_whitelist_verify_amd(0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "whitelist_verify.c"), "-o", str(tmp_path / "e.o")], check=True)
