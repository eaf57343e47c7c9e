"""CPU tier: public-key conversion, negation, tweak-mul and combine.  secp256k1_zkp_amd/csrc/pubkey.h runs on the host
(tests/host_emul/pubkey_emu.cpp, S2K_VERIFY on, 12-bit generator table; combine through the same plan the engine uses) against the
recorded vectors (tests/golden/pubkey_vectors.json) and the unmodified reference rebuilt now (oracle/_ref through tests/pubkey_ref.py);
plus the ABI, the argument checks that run in front of any device, the build entry and the C example."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PK_BYTES = {0: 32, 1: 64, 2: 33, 3: 65, 4: 64, 5: 64}
PUBKEY_SYMBOLS = ["secp256k1_ec_pubkey_convert_batch", "secp256k1_ec_pubkey_convert_batch_dev", "secp256k1_ec_pubkey_negate_batch", "secp256k1_ec_pubkey_negate_batch_dev",
                  "secp256k1_ec_pubkey_tweak_mul_batch", "secp256k1_ec_pubkey_tweak_mul_batch_dev", "secp256k1_ec_pubkey_tweak_mul_batch_group",
                  "secp256k1_ec_pubkey_combine_batch", "secp256k1_ec_pubkey_combine_batch_dev",
                  "secp256k1_ec_pubkey_parse_amd", "secp256k1_ec_pubkey_serialize_amd", "secp256k1_ec_pubkey_negate_amd", "secp256k1_ec_pubkey_tweak_mul_amd",
                  "secp256k1_ec_pubkey_combine_amd", "secp256k1_xonly_pubkey_parse_amd", "secp256k1_xonly_pubkey_serialize_amd", "secp256k1_xonly_pubkey_from_pubkey_amd"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_pubkey_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_pubkey_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.emu_pubkey_convert.argtypes = [vp, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.emu_pubkey_tweak_mul.argtypes = [vp, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
    lib.emu_pubkey_combine.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_char_p, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_uint, vp]
    lib.emu_pubkey_bytes.restype = ctypes.c_size_t
    lib.emu_pubkey_fanin_default.restype = ctypes.c_uint
    return lib


@pytest.fixture(scope="module")
def pref(ref):
    from tests.pubkey_ref import PubkeyRef
    return PubkeyRef()


@pytest.fixture(scope="module")
def golden():
    from tests.pubkey_ref import from_json
    return from_json(json.load(open(os.path.join(HERE, "golden", "pubkey_vectors.json")))["vectors"])


def _edge_only(items):
    return {k: [x for x in v if not x[0].startswith("random ")] for k, v in items.items()}


def _run_convert(emu, items):
    for name, fmt, key, v, outs, par, nouts, npar in items:
        for neg, eo, ep in ((0, outs, par), (1, nouts, npar)):
            for of in range(6):
                o = ctypes.create_string_buffer(b"\xff" * PK_BYTES[of], PK_BYTES[of]); p = ctypes.create_string_buffer(b"\xff", 1)
                assert emu.emu_pubkey_convert(o, of, p, key, fmt, neg) == v, (name, neg, of)
                assert o.raw == eo[of] and p.raw[0] == ep, (name, neg, of)
        o = ctypes.create_string_buffer(64)
        assert emu.emu_pubkey_convert(o, 1, None, key, fmt, 0) == v and o.raw == outs[1], name          # no parity wanted


def _run_tweak_mul(emu, items, out_formats=range(6)):
    for name, fmt, key, t, v, outs, par in items:
        for of in out_formats:
            o = ctypes.create_string_buffer(b"\xff" * PK_BYTES[of], PK_BYTES[of]); p = ctypes.create_string_buffer(b"\xff", 1)
            assert emu.emu_pubkey_tweak_mul(o, of, p, key, fmt, t) == v, (name, of)
            assert o.raw == outs[of] and p.raw[0] == par, (name, of)


def _combine_batch(emu, items, fmt, out_format, fanin):
    """the items of ONE key format as one ragged batch -> (results, outs, parities, passes)"""
    keys = b"".join(b"".join(x[2]) for x in items)
    off = np.zeros(len(items) + 1, np.uint64); off[1:] = np.cumsum([len(x[2]) for x in items])
    n = len(items); ob = PK_BYTES[out_format]
    res = np.full(n, 7, np.int32); out = np.full((n, ob), 0xFF, np.uint8); par = np.full(n, 0xFF, np.uint8); passes = ctypes.c_size_t(0)
    assert emu.emu_pubkey_combine(res.ctypes.data, out.ctypes.data, out_format, par.ctypes.data, keys, fmt, off.ctypes.data, n, fanin, ctypes.byref(passes)) == 1
    return res, out, par, passes.value


def _run_combine(emu, items, fanins, out_formats=(1, 2)):
    for fmt in range(5):
        sub = [x for x in items if x[1] == fmt]
        if not sub:
            continue
        for fanin in fanins:
            for of in out_formats:
                res, out, par, _ = _combine_batch(emu, sub, fmt, of, fanin)
                for i, x in enumerate(sub):
                    assert res[i] == x[3] and out[i].tobytes() == x[4][of] and par[i] == x[5], (x[0], fmt, fanin, of)


def test_golden_fixture_shape(golden):
    conv = {x[0]: x for x in golden["convert"]}; tm = {x[0]: x for x in golden["tweak_mul"]}; comb = {x[0]: x for x in golden["combine"]}
    for d, v in ((conv, golden["convert"]), (tm, golden["tweak_mul"]), (comb, golden["combine"])):
        assert len(d) == len(v) and sum(1 for k in d if k.startswith("random ")) == 64
    assert {x[1] for x in golden["convert"]} == {0, 1, 2, 3, 4} == {x[1] for x in golden["tweak_mul"]} == {x[1] for x in golden["combine"]}
    assert conv["all-zero object"][3] == 0 and not any(conv["all-zero object"][4][1])
    odd = conv["object with odd y (to format 5: y is made even)"]
    assert odd[3] == 1 and odd[5] == 1 and odd[4][1][32] & 1 == 1 and odd[4][5][32] & 1 == 0 and odd[4][5][:32] == odd[4][1][:32] and odd[7] == 0
    for nm in ("fmt 0 x = p", "fmt 0 x = 0", "fmt 2 bad prefix 04", "fmt 3 bad prefix 02", "fmt 3 prefix 06 with odd y", "fmt 3 prefix 07 with even y", "fmt 3 y = p",
               "fmt 4 y = p", "fmt 4 y off the curve", "fmt 4 y = 2^256 - 1", "fmt 4 x = p"):
        assert conv[nm][3] == 0, nm
    for nm in ("fmt 3 prefix 07 with odd y", "fmt 3 prefix 06 with even y", "fmt 3 y replaced by p - y", "fmt 4 y replaced by p - y", "valid odd y hybrid"):
        assert conv[nm][3] == 1, nm
    assert [tm[f"key 0 fmt 1 tweak {s}"][4] for s in ("0", "1", "2", "n-1", "n", "n+1", "2^256-1", "lambda", "2^128")] == [0, 1, 1, 1, 0, 0, 0, 1, 1]
    assert tm["key 0 fmt 1 tweak 1"][5][1] == tm["key 0 fmt 1 tweak 1"][2]                 # t = 1 leaves the key as it is
    assert [comb[s][3] for s in ("0 keys", "1 keys", "[P, P]", "[P, Q, P+Q]", "[P, -P]", "[P, -P, Q]", "[P, Q, -(P+Q)]")] == [0, 1, 1, 1, 0, 1, 0]
    assert comb["[P, -P, Q]"][4][1] == comb["[P, -P, Q]"][2][2]
    assert comb["2F keys, the second chunk negates the first"][3] == 0 and comb["2F keys, the second chunk repeats the first"][3] == 1
    assert {len(x[2]) for x in golden["combine"]} >= {0, 1, 2, 3, 15, 16, 17, 33, 257}
    assert all(x[3] == 0 for x in golden["combine"] if x[0].startswith("refused key"))


def test_emu_golden(emu, golden):
    """the recorded vectors (no reference needed): every input format to every output format, plain and negated"""
    assert emu.emu_pubkey_fanin_default() == 16 and [emu.emu_pubkey_bytes(f) for f in range(6)] == [32, 64, 33, 65, 64, 64]
    _run_convert(emu, golden["convert"])
    _run_tweak_mul(emu, golden["tweak_mul"])
    _run_combine(emu, golden["combine"], (16, 2, 3))


def test_emu_combine_plan_depth(emu, golden):
    """one chunk per set is one pass; F + 1 keys two; F * F + 1 keys three (F = 16), and F = 2 walks 9 keys through four"""
    by = {x[0]: x for x in golden["combine"]}
    for names, fanin, passes in ((["1 keys", "16 keys", "0 keys"], 16, 1), (["17 keys", "1 keys"], 16, 2), (["257 keys"], 16, 3), (["9 keys"], 2, 4), (["2 keys"], 2, 1)):
        sub = [by[n] for n in names]
        res, out, par, got = _combine_batch(emu, sub, 1, 1, fanin)
        assert got == passes and res.tolist() == [x[3] for x in sub] and [o.tobytes() for o in out] == [x[4][1] for x in sub], (names, fanin)


def test_emu_refuses_unknown_formats(emu):
    o = ctypes.create_string_buffer(65)
    for of, f in ((6, 1), (-1, 1), (1, 5), (1, -1), (1, 6)):
        assert emu.emu_pubkey_convert(o, of, None, bytes(65), f, 0) == -1
        assert emu.emu_pubkey_tweak_mul(o, of, None, bytes(65), f, bytes(32)) == -1
    off = np.array([0, 1], np.uint64); res = np.zeros(1, np.int32)
    for of, f, fan in ((6, 1, 16), (1, 5, 16), (1, 1, 1), (1, 1, 65)):
        assert emu.emu_pubkey_combine(res.ctypes.data, o, of, None, bytes(65), f, off.ctypes.data, 1, fan, None) == 0


def test_emu_edge_list_against_reference(emu, pref, golden):
    """the edge lists rebuilt now; the recorded vectors are the reference's of today"""
    from tests.pubkey_ref import edge_cases
    cases = edge_cases(pref)
    _run_convert(emu, cases["convert"])
    _run_tweak_mul(emu, cases["tweak_mul"], (1, 2))
    _run_combine(emu, cases["combine"], (16,), (1,))
    assert cases == _edge_only(golden)


def test_emu_random_against_reference(emu, pref):
    """128 seeded items per call, every fourth one corrupted"""
    from tests.pubkey_ref import random_items
    items = random_items(pref, 128, 7705)
    for k, col in (("convert", 3), ("tweak_mul", 4), ("combine", 3)):
        ones = sum(x[col] for x in items[k])
        assert ones >= 16 and 128 - ones >= 8, (k, ones)
    _run_convert(emu, items["convert"])
    _run_tweak_mul(emu, items["tweak_mul"], (1, 4))
    _run_combine(emu, items["combine"], (16, 2), (1,))


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    units = build_lib.UNITS + build_lib.UNITS_ADDED
    assert "engine_pubkey" in units and units.index("engine_pubkey") < units.index("engine_schnorr_all")
    assert os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "engine_pubkey.hip")) and os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "pubkey.h"))
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in PUBKEY_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    for i, nm in enumerate(("XONLY", "OBJECT", "COMPRESSED", "FULL", "AFFINE", "XONLY_OBJECT")):
        assert ("#define S2K_PK_%s %d\n" % (nm, i)) in hdr
    assert "#define S2K_OPT_PUBKEY_FOLD_FANIN 15\n" in hdr and "#define S2K_OPT_MUSIG_SUM_FANIN 12\n" in hdr
    from secp256k1_zkp_amd import api
    assert api.Engine.OPT_PUBKEY_FOLD_FANIN == 15
    for m in ("pubkey_convert", "pubkey_negate", "pubkey_tweak_mul", "pubkey_combine"):
        assert callable(getattr(api.Engine, m)) and callable(getattr(api.Engine, m + "_dev")), m
    assert callable(api.Group.pubkey_tweak_mul)


def test_library_exports_pubkey():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in PUBKEY_SYMBOLS:
        assert hasattr(lib, name) and (" T " + name + "\n") in out, name
    # NULL engine / group: the call fails with a message, whatever the device situation
    for name in ("secp256k1_ec_pubkey_convert_batch", "secp256k1_ec_pubkey_negate_batch"):
        assert getattr(lib, name)(None, None, None, 1, None, None, 1, 1) == 0 and "null engine" in _native.last_error()
        assert getattr(lib, name + "_dev")(None, None, None, None, 1, None, None, 1, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ec_pubkey_tweak_mul_batch(None, None, None, 1, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ec_pubkey_tweak_mul_batch_dev(None, None, None, None, 1, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ec_pubkey_tweak_mul_batch_group(None, None, None, 1, None, None, 1, None, 1) == 0 and "null group" in _native.last_error()
    assert lib.secp256k1_ec_pubkey_combine_batch(None, None, None, 1, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ec_pubkey_combine_batch_dev(None, None, None, None, 1, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()


def test_single_item_forms_check_their_arguments_first():
    """NULL where the reference has ARG_CHECK is an illegal argument before any device is touched, and the outputs the reference zeroes
    in front of that check are zeroed"""
    from secp256k1_zkp_amd import _native
    lib = _native.load()
    S = lib.s2k_last_status
    obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_ec_pubkey_parse_amd(None, None, bytes(33), 33) == 0 and S() == 2
    assert lib.secp256k1_ec_pubkey_parse_amd(None, obj, None, 33) == 0 and S() == 2 and obj.raw == bytes(64)
    obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
    for ln in (0, 32, 34, 64, 66):                                                        # no such encoding: 0 without a launch, and no error
        assert lib.secp256k1_ec_pubkey_parse_amd(None, obj, bytes(66), ln) == 0 and S() == 0 and obj.raw == bytes(64)
    out = ctypes.create_string_buffer(b"\xff" * 65, 65)
    ln = ctypes.c_size_t(65)
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, out, None, bytes(64), 258) == 0 and S() == 2
    ln.value = 32
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, out, ctypes.byref(ln), bytes(64), 258) == 0 and S() == 2 and ln.value == 32 and out.raw == b"\xff" * 65
    ln.value = 64
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, out, ctypes.byref(ln), bytes(64), 2) == 0 and S() == 2 and ln.value == 64
    ln.value = 65
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, None, ctypes.byref(ln), bytes(64), 2) == 0 and S() == 2 and ln.value == 0
    ln.value = 40
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, out, ctypes.byref(ln), None, 258) == 0 and S() == 2 and ln.value == 0 and out.raw == bytes(40) + b"\xff" * 25
    ln.value = 65
    assert lib.secp256k1_ec_pubkey_serialize_amd(None, out, ctypes.byref(ln), bytes(64), 1) == 0 and S() == 2 and ln.value == 0       # flags of another type
    assert lib.secp256k1_ec_pubkey_negate_amd(None, None) == 0 and S() == 2
    assert lib.secp256k1_ec_pubkey_tweak_mul_amd(None, None, bytes(32)) == 0 and S() == 2
    obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_ec_pubkey_tweak_mul_amd(None, obj, None) == 0 and S() == 2 and obj.raw == b"\xff" * 64
    key = ctypes.create_string_buffer(b"\x01" * 64, 64)
    ptrs = (ctypes.c_void_p * 2)(ctypes.addressof(key), None)
    assert lib.secp256k1_ec_pubkey_combine_amd(None, None, ptrs, 1) == 0 and S() == 2
    for args in ((ptrs, 0), (None, 1), (ptrs, 2)):                                        # n >= 1, the array, every pointer
        obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
        assert lib.secp256k1_ec_pubkey_combine_amd(None, obj, *args) == 0 and S() == 2 and obj.raw == bytes(64)
    assert lib.secp256k1_xonly_pubkey_parse_amd(None, None, bytes(32)) == 0 and S() == 2
    obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_xonly_pubkey_parse_amd(None, obj, None) == 0 and S() == 2 and obj.raw == bytes(64)
    o32 = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert lib.secp256k1_xonly_pubkey_serialize_amd(None, None, bytes(64)) == 0 and S() == 2
    assert lib.secp256k1_xonly_pubkey_serialize_amd(None, o32, None) == 0 and S() == 2 and o32.raw == bytes(32)
    par = ctypes.c_int(9)
    assert lib.secp256k1_xonly_pubkey_from_pubkey_amd(None, None, ctypes.byref(par), bytes(64)) == 0 and S() == 2
    obj = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.secp256k1_xonly_pubkey_from_pubkey_amd(None, obj, ctypes.byref(par), None) == 0 and S() == 2 and obj.raw == b"\xff" * 64 and par.value == 9


def test_python_argument_checks():
    """the size, format and offset checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    g = api.Group.__new__(api.Group)
    for m in (e.pubkey_convert, e.pubkey_negate):
        for args in ((bytes(64), 5, 1), (bytes(64), 1, 6), (bytes(64), -1, 1), (bytes(63), 1, 1), (bytes(33), 3, 1), (None, 1, 1)):
            with pytest.raises(ValueError):
                m(*args)
    for obj in (e, g):
        for args, kw in (((bytes(64), bytes(32)), dict(key_format=5)), ((bytes(64), bytes(32)), dict(out_format=6)), ((bytes(33), bytes(32)), dict(key_format=1)),
                         ((bytes(64), bytes(31)), {}), ((None, bytes(32)), {}), ((bytes(64), None), {})):
            with pytest.raises(ValueError):
                obj.pubkey_tweak_mul(*args, **kw)
    for off in ([], [1, 2], [0, 2, 1], [0, 3], None):                                     # empty, not starting at 0, decreasing, past the keys, missing
        with pytest.raises(ValueError):
            e.pubkey_combine(bytes(128), off)
    for kw in (dict(key_format=5), dict(out_format=6), dict(key_format=-1)):
        with pytest.raises(ValueError):
            e.pubkey_combine(bytes(128), [0, 2], **kw)
    with pytest.raises(ValueError):
        e.pubkey_combine(None, [0, 0])
    for off in ([], [1, 2], [0, 2, 1], None):
        with pytest.raises(ValueError):
            e.pubkey_combine_dev(None, None, None, off)
    with pytest.raises(ValueError):
        e.pubkey_convert_dev(None, None, None, 5, 1)


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { size_t n = 33; return secp256k1_ec_pubkey_convert_batch(0, 0, 0, S2K_PK_COMPRESSED, 0, 0, S2K_PK_AFFINE, 0) + '
                   'secp256k1_ec_pubkey_negate_batch(0, 0, 0, S2K_PK_XONLY_OBJECT, 0, 0, S2K_PK_OBJECT, 0) + '
                   'secp256k1_ec_pubkey_tweak_mul_batch(0, 0, 0, S2K_PK_OBJECT, 0, 0, S2K_PK_FULL, 0, 0) + '
                   'secp256k1_ec_pubkey_combine_batch(0, 0, 0, S2K_PK_XONLY, 0, 0, S2K_PK_OBJECT, 0, 0) + secp256k1_ec_pubkey_serialize_amd(0, 0, &n, 0, 258) + '
                   'secp256k1_ec_pubkey_combine_amd(0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "pubkey_combine.c"), "-o", str(tmp_path / "e.o")], check=True)
