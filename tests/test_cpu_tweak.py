"""CPU tier: Taproot tweak checks and public-key tweak-add.  secp256k1_zkp_amd/csrc/tweak.h runs on the host
(tests/host_emul/tweak_emu.cpp, S2K_VERIFY on, 12-bit generator table) against the unmodified reference (oracle/_ref through
tests/tweak_ref.py) and the recorded vectors (tests/golden/tweak_vectors.json); plus the ABI, the argument checks and the C example."""
import ctypes
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TWEAK_SYMBOLS = ["secp256k1_xonly_pubkey_tweak_add_check_batch", "secp256k1_xonly_pubkey_tweak_add_check_batch_dev",
                 "secp256k1_xonly_pubkey_tweak_add_check_batch_group", "secp256k1_pubkey_tweak_add_batch", "secp256k1_pubkey_tweak_add_batch_dev",
                 "secp256k1_xonly_pubkey_tweak_add_check_amd", "secp256k1_xonly_pubkey_tweak_add_amd", "secp256k1_ec_pubkey_tweak_add_amd"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_tweak_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_tweak_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_tweak_check.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    lib.emu_tweak_add.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    lib.emu_tweak_gmul.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.emu_tweak_gtab_bits.restype = ctypes.c_uint
    return lib


@pytest.fixture(scope="module")
def tref(ref):
    from tests.tweak_ref import TweakRef
    return TweakRef()


def golden():
    from tests.tweak_ref import from_json
    return from_json(json.load(open(os.path.join(HERE, "golden", "tweak_vectors.json")))["vectors"])


def _run_items(emu, items):
    """every item through the host-emulated lane routines: the verdicts, and for the add form the output object byte for byte"""
    for name, fmt, key, t, tw, par, cv, av, out in items:
        if cv is not None:
            assert emu.emu_tweak_check(tw, par, key, fmt, t) == cv, name
        if av is not None:
            o = ctypes.create_string_buffer(b"\xff" * 64, 64)
            assert emu.emu_tweak_add(o, key, fmt, t) == av, name
            assert o.raw == out, name


def test_golden_fixture_shape():
    v = golden()
    names = {x[0]: x for x in v}
    assert len(names) == len(v) and sum(1 for x in v if x[0].startswith("random ")) == 64
    assert {x[1] for x in v} == {0, 1, 2}
    assert {x[5] for x in v if x[6] == 1} == {0, 1}                                      # valid checks of both parities
    assert {x[5] for x in v} >= {0, 1, 2, 255}
    assert names["P = kG, t = n-k, fmt 1"][6:] == (0, 0, bytes(64)) and names["P = kG, t = k, fmt 1"][6:8] == (1, 1)
    assert names["-P = kG, t = n-k, fmt 1"][7] == 1 and names["-P = kG, t = k, fmt 1"][7] == 0
    assert names["tweak 0 fmt 1"][7] == 1 and names["tweak 0 fmt 1"][8] == names["tweak 0 fmt 1"][2]     # t = 0 leaves the key as it is
    assert [names[f"tweak {s} fmt 2"][7] for s in ("0", "1", "n-1", "n", "n+1", "2^256-1")] == [1, 1, 1, 0, 0, 0]
    assert names["fmt 1 all-zero object"][6:] == (0, 0, bytes(64))
    assert names["fmt 1 object with odd y, t = 0"][8][32] & 1 == 1
    assert names["fmt 0 x = p"][6:8] == (0, 0) and names["fmt 0 x = 0"][6:8] == (0, 0) and names["fmt 2 bad prefix 04"][7] == 0


def test_emu_golden(emu):
    """the recorded vectors (no reference needed)"""
    assert emu.emu_tweak_gtab_bits() == 12
    _run_items(emu, golden())


def test_emu_edge_list_against_reference(emu, tref):
    """the edge list rebuilt now; the recorded vectors are the reference's of today"""
    from tests.tweak_ref import edge_cases
    cases = edge_cases(tref)
    _run_items(emu, cases)
    assert cases == [x for x in golden() if not x[0].startswith("random ")]


def test_emu_random_against_reference(emu, tref):
    """256 seeded items, every fourth one corrupted; each verdict occurs in at least one eighth of them"""
    from tests.tweak_ref import random_items
    items = random_items(tref, 256, 4403)
    ones = sum(x[6] for x in items)
    assert ones >= 32 and 256 - ones >= 32
    _run_items(emu, items)


def test_emu_fixed_base_against_reference(emu, tref):
    """t * G from tweak_gmul_fixed against secp256k1_ec_pubkey_create at the recoding boundaries of every table width"""
    from tests.tweak_ref import boundary_tweaks, b32, N
    ts = [t for _, _, t in boundary_tweaks()] + [1, 2, N - 1, (1 << 255) + 12345]
    for t in ts:
        xy = ctypes.create_string_buffer(64)
        assert emu.emu_tweak_gmul(xy, b32(t)) == 0, hex(t)
        obj = tref.ec_create(b32(t))
        assert xy.raw == obj[31::-1] + obj[:31:-1], hex(t)
    xy = ctypes.create_string_buffer(64)
    assert emu.emu_tweak_gmul(xy, b32(0)) == 1                                           # infinity


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_tweak" in build_lib.UNITS + build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in TWEAK_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name


def test_library_exports_tweak():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in TWEAK_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine / group: the call fails with a message, whatever the device situation
    assert lib.secp256k1_xonly_pubkey_tweak_add_check_batch(None, None, None, None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_xonly_pubkey_tweak_add_check_batch_dev(None, None, None, None, None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_pubkey_tweak_add_batch(None, None, None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_pubkey_tweak_add_batch_dev(None, None, None, None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_xonly_pubkey_tweak_add_check_batch_group(None, None, None, None, None, 0, None, 1) == 0 and "null group" in _native.last_error()
    # the single-item forms: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched
    assert lib.secp256k1_xonly_pubkey_tweak_add_check_amd(None, None, 0, None, None) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_xonly_pubkey_tweak_add_amd(None, None, None, None) == 0 and lib.s2k_last_status() == 2
    out = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_xonly_pubkey_tweak_add_amd(None, out, None, None) == 0 and lib.s2k_last_status() == 2 and out.raw == bytes(64)      # zeroed first, as the reference
    assert lib.secp256k1_ec_pubkey_tweak_add_amd(None, None, None) == 0 and lib.s2k_last_status() == 2
    # a parity that is neither 0 nor 1: 0 without a launch, and no error
    key = ctypes.create_string_buffer(b"\x01" * 64, 64)
    assert lib.secp256k1_xonly_pubkey_tweak_add_check_amd(None, bytes(32), 2, key, bytes(32)) == 0 and lib.s2k_last_status() == 0


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    g = api.Group.__new__(api.Group)
    for obj in (e, g):
        with pytest.raises(ValueError):
            obj.xonly_tweak_add_check_batch(bytes(32), bytes(1), bytes(33), bytes(32), key_format=2)      # the check form takes no compressed keys
        with pytest.raises(ValueError):
            obj.xonly_tweak_add_check_batch(bytes(32), bytes(1), bytes(32), bytes(32), key_format=3)
        with pytest.raises(ValueError):
            obj.xonly_tweak_add_check_batch(bytes(32), bytes(1), bytes(32), bytes(32), key_format=1)      # objects are 64 bytes
        with pytest.raises(ValueError):
            obj.xonly_tweak_add_check_batch(bytes(32), bytes(2), bytes(32), bytes(32))                    # one parity byte per item
        with pytest.raises(ValueError):
            obj.xonly_tweak_add_check_batch(None, bytes(1), bytes(32), bytes(32))
    with pytest.raises(ValueError):
        e.pubkey_tweak_add_batch(bytes(64), bytes(32), key_format=3)
    with pytest.raises(ValueError):
        e.pubkey_tweak_add_batch(bytes(64), bytes(32), key_format=2)                                      # compressed keys are 33 bytes
    with pytest.raises(ValueError):
        e.pubkey_tweak_add_batch(None, bytes(32))


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_xonly_pubkey_tweak_add_check_batch(0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_pubkey_tweak_add_batch(0, 0, 0, 0, 0, 0, 0) + secp256k1_ec_pubkey_tweak_add_amd(0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "tweak_check.c"), "-o", str(tmp_path / "e.o")], check=True)
