"""CPU tier: asset generators and explicit-amount commitments.  secp256k1_zkp_amd/csrc/generator.h runs on the host
(tests/host_emul/generator_emu.cpp, S2K_VERIFY on, 12-bit generator table) against the unmodified reference (oracle/_ref through
tests/generator_ref.py), against the plain-Python model of the map where the reference keeps it static, and against the recorded
vectors (tests/golden/generator_vectors.json); plus the ABI, the argument checks and the C example."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GEN_SYMBOLS = ["secp256k1_generator_generate_batch", "secp256k1_generator_generate_batch_dev", "secp256k1_generator_parse_batch",
               "secp256k1_generator_parse_batch_dev", "secp256k1_generator_serialize_batch", "secp256k1_generator_serialize_batch_dev",
               "secp256k1_pedersen_commit_batch", "secp256k1_pedersen_commit_batch_dev", "secp256k1_generator_generate_amd",
               "secp256k1_generator_parse_amd", "secp256k1_pedersen_commit_amd"]
MODEL_SEED = 5503          # 512 plain + 64 blinded keys; the branch counts over their 1 024 + 128 maps are asserted below


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_generator_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_generator_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    cp = ctypes.c_char_p
    lib.emu_gen_map.argtypes = [cp, cp]
    lib.emu_gen_from_t.argtypes = [cp, cp, cp, cp]
    lib.emu_gen_generate.argtypes = [cp, cp, cp]
    lib.emu_gen_parse.argtypes = [cp, cp]
    lib.emu_gen_serialize.argtypes = [cp, cp]; lib.emu_gen_serialize.restype = None
    lib.emu_pedersen_commit.argtypes = [cp, cp, ctypes.c_ulonglong, cp]
    return lib


@pytest.fixture(scope="module")
def gref(ref):
    from tests.generator_ref import GeneratorRef
    return GeneratorRef()


@pytest.fixture(scope="module")
def model_keys():
    """(512 keys, 64 (key, blind) pairs) from the fixed seed"""
    rng = np.random.default_rng(MODEL_SEED)
    keys = [bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()) for _ in range(512)]
    blinded = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()), bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())) for _ in range(64)]
    return keys, blinded


def golden():
    from tests.generator_ref import from_json
    return from_json(json.load(open(os.path.join(HERE, "golden", "generator_vectors.json")))["vectors"])


def _run_items(emu, items):
    """every item through the host-emulated lane routine of its entry point: verdict and output byte for byte"""
    for op, name, args, v, out in items:
        if op == "parse":
            o = ctypes.create_string_buffer(b"\xff" * 64, 64)
            got = emu.emu_gen_parse(o, args[0])
        elif op == "serialize":
            o = ctypes.create_string_buffer(b"\xff" * 33, 33)
            emu.emu_gen_serialize(o, args[0]); got = 1
        elif op == "generate":
            o = ctypes.create_string_buffer(b"\xff" * 64, 64)
            got = emu.emu_gen_generate(o, args[0], args[1])
        else:
            o = ctypes.create_string_buffer(b"\xff" * 33, 33)
            got = emu.emu_pedersen_commit(o, args[0], args[1], args[2])
        assert got == v, (op, name)
        assert o.raw == out, (op, name)


def test_model_against_reference(gref, model_keys):
    """the Python generate equals the reference's on all 512 keys and all 64 blinded items, and the maps behind them take every branch
    at least 128 times"""
    from tests.generator_ref import model_generate
    keys, blinded = model_keys
    counts = [0, 0, 0]
    for k in keys:
        v, out, br = model_generate(k)
        assert (v, out) == gref.generate(k) and v == 1
        counts[br[0]] += 1; counts[br[1]] += 1
    assert sum(counts) == 1024 and min(counts) >= 128, counts
    for k, b in blinded:
        v, out, _ = model_generate(k, b)
        assert (v, out) == gref.generate(k, b) and v == 1


def _map_check(emu, t):
    from tests.generator_ref import model_map, b32
    x, y, br = model_map(t)
    o = ctypes.create_string_buffer(64)
    assert emu.emu_gen_map(o, b32(t)) == br, hex(t)
    assert o.raw == b32(x) + b32(y), hex(t)
    return br


def test_emu_map_against_model(emu, model_keys):
    """the emulated map on the 1 024 t values behind the model test, on t in {0, 1, 2, p-1, p-2}, and on one odd and one even t per branch"""
    from tests.generator_ref import model_hash_t, model_map, P, D, b32
    keys, _ = model_keys
    seen = set()
    for k in keys:
        for t in model_hash_t(k):
            seen.add((_map_check(emu, t), t & 1))
    assert seen == {(b, o) for b in range(3) for o in range(2)}
    for t in (0, 1, 2, P - 1, P - 2):
        _map_check(emu, t)
    assert model_map(0)[0] == D                                                 # j == 0: the point (d, f(d))
    assert emu.emu_gen_map(ctypes.create_string_buffer(64), b32(P)) == -1


def test_emu_generate_pairs_against_model(emu, model_keys):
    """the lane routine at chosen (t1, t2): equal (the doubling), opposite (0 and zero bytes), one of them 0, with and without a blind"""
    from tests.generator_ref import model_hash_t, model_from_t, P, b32
    keys, blinded = model_keys
    t1, t2 = model_hash_t(keys[0])
    blind = int.from_bytes(blinded[0][1], "big")
    cases = [("equal", t1, t1), ("opposite", t1, P - t1), ("opposite 2", P - t2, t2), ("first 0", 0, t2), ("second 0", t1, 0), ("both 0", 0, 0),
             ("ordinary", t1, t2)]
    for name, a, b in cases:
        for bl in (None, blind, 0):
            v, out, _ = model_from_t(a, b, bl)
            o = ctypes.create_string_buffer(b"\xff" * 64, 64)
            got = emu.emu_gen_from_t(o, b32(a), b32(b), None if bl is None else b32(bl))
            assert (got, o.raw) == (v, out), (name, bl)
            if name.startswith("opposite"):
                assert (v == 0 and out == bytes(64)) if not bl else v == 1      # with a blind the sum is blind * G: finite
            else:
                assert v == 1


def test_golden_fixture_shape():
    v = golden()
    names = {x[1]: x for x in v}
    assert len(names) == len(v)
    for op in ("parse", "serialize", "generate", "commit"):
        assert sum(1 for x in v if x[0] == op and x[1].startswith("random ")) == 64
        assert {x[3] for x in v if x[0] == op} == ({1} if op == "serialize" else {0, 1})
    assert all(not any(x[4]) for x in v if x[3] == 0)
    assert [names[f"prefix {p:02x} refused"][3] for p in (0x00, 0x02, 0x08, 0x09, 0x0c, 0xff)] == [0] * 6
    assert names["prefix 0a valid x"][3] == 1 and names["prefix 0b valid x"][3] == 1
    assert names["x = p prefix 0a"][3] == 0 and names["x = p+1 prefix 0a"][3] == 0 and names["x = 2^256-1 prefix 0b"][3] == 0
    assert [names[f"blind {s}"][3] for s in ("0", "1", "n-1", "n", "n+1", "2^256-1")] == [1, 1, 1, 0, 0, 0]
    assert names["kG value 0 NULL blinds"][3] == 0 and names["kG value 1 blind n"][3] == 0
    assert any("infinity" in n for n in names) and any("doubling" in n for n in names)
    assert os.path.getsize(os.path.join(HERE, "golden", "generator_vectors.json")) < 200_000


def test_emu_golden(emu):
    """the recorded vectors (no reference needed)"""
    _run_items(emu, golden())


def test_emu_edge_list_against_reference(emu, gref):
    """the edge list rebuilt now; the recorded vectors are the reference's of today; parse of serialize is the identity in the emulation too"""
    from tests.generator_ref import edge_cases
    cases = edge_cases(gref)
    _run_items(emu, cases)
    assert cases == [x for x in golden() if not x[1].startswith("random ")]
    for op, name, args, v, out in cases:
        if op == "serialize":
            o = ctypes.create_string_buffer(64)
            assert emu.emu_gen_parse(o, out) == 1 and o.raw == args[0], name


def test_emu_random_against_reference(emu, gref):
    """128 seeded items per entry point, asked of the reference now"""
    from tests.generator_ref import random_items
    items = random_items(gref, 128, 5504)
    for op in ("parse", "generate", "commit"):
        zeros = sum(1 for x in items if x[0] == op and x[3] == 0)
        assert 8 <= zeros <= 96, (op, zeros)
    _run_items(emu, items)


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_generator" in build_lib.UNITS + build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in GEN_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name


def test_library_exports_generator():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in GEN_SYMBOLS:
        assert hasattr(lib, name), name
    # NULL engine: the call fails with a message, whatever the device situation
    assert lib.secp256k1_generator_generate_batch(None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_generator_generate_batch_dev(None, None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_generator_parse_batch(None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_generator_parse_batch_dev(None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_generator_serialize_batch(None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_generator_serialize_batch_dev(None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_pedersen_commit_batch(None, None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_pedersen_commit_batch_dev(None, None, None, None, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    # the single-item forms: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched; outputs zeroed first
    out = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_generator_generate_amd(None, None, bytes(32)) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_generator_generate_amd(None, out, None) == 0 and lib.s2k_last_status() == 2 and out.raw == bytes(64)
    out = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_generator_parse_amd(None, None, bytes(33)) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_generator_parse_amd(None, out, None) == 0 and lib.s2k_last_status() == 2 and out.raw == bytes(64)
    out = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_pedersen_commit_amd(None, None, bytes(32), 1, bytes(64)) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_pedersen_commit_amd(None, out, None, 1, bytes(64)) == 0 and lib.s2k_last_status() == 2 and out.raw == bytes(64)
    assert lib.secp256k1_pedersen_commit_amd(None, out, bytes(32), 1, None) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    with pytest.raises(ValueError):
        e.generator_generate_batch(None)
    with pytest.raises(ValueError):
        e.generator_generate_batch(bytes(33))
    with pytest.raises(ValueError):
        e.generator_generate_batch(bytes(64), bytes(32))                # one blind per key
    with pytest.raises(ValueError):
        e.generator_parse_batch(bytes(34))
    with pytest.raises(ValueError):
        e.generator_parse_batch(None)
    with pytest.raises(ValueError):
        e.generator_serialize_batch(bytes(63))
    with pytest.raises(ValueError):
        e.pedersen_commit_batch([1, 2], bytes(64))                      # one generator object per value
    with pytest.raises(ValueError):
        e.pedersen_commit_batch([1], bytes(64), bytes(31))
    with pytest.raises(ValueError):
        e.pedersen_commit_batch(None, bytes(64))


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_generator_generate_batch(0, 0, 0, 0, 0, 0) + '
                   'secp256k1_generator_parse_batch(0, 0, 0, 0, 0) + secp256k1_generator_serialize_batch(0, 0, 0, 0) + '
                   'secp256k1_pedersen_commit_batch(0, 0, 0, 0, 0, 0, 0) + secp256k1_pedersen_commit_amd(0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "asset_commit.c"), "-o", str(tmp_path / "e.o")], check=True)
