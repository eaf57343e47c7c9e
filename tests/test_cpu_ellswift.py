"""CPU tier: ElligatorSwift decoding and encoding.  secp256k1_zkp_amd/csrc/ellswift.h runs on the host (tests/host_emul/ellswift_emu.cpp,
S2K_VERIFY on) against the recorded answers of the reference (tests/golden/ellswift_vectors.json: the module's own vectors and what
secp256k1_ellswift_decode / _encode returned) and against the Python model of tests/ellswift_ref.py; plus the counter schedule past the
first pool, the attempt cap, the sanitizer program, the ABI, the argument checks and the C example."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess

import pytest

from tests import ellswift_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ELLSWIFT_SYMBOLS = ["secp256k1_ellswift_decode_batch", "secp256k1_ellswift_decode_batch_dev", "secp256k1_ellswift_decode_batch_group",
                    "secp256k1_ellswift_encode_batch", "secp256k1_ellswift_encode_batch_dev", "secp256k1_ellswift_decode_amd", "secp256k1_ellswift_encode_amd",
                    "s2k_engine_ellswift_capped"]
OUT_BYTES = {0: 32, 1: 64, 2: 33}


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ellswift_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ellswift_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    cp = ctypes.c_char_p
    lib.emu_ellswift_decode.argtypes = [cp, ctypes.c_int, cp]
    lib.emu_ellswift_decode.restype = None
    lib.emu_ellswift_which.argtypes = [cp, ctypes.c_int]
    lib.emu_ellswift_inv.argtypes = [cp, cp, cp, ctypes.c_int]
    lib.emu_ellswift_encode.argtypes = [cp, ctypes.POINTER(ctypes.c_int), cp, ctypes.c_int, cp, ctypes.c_uint]
    lib.emu_ellswift_schedule.argtypes = [ctypes.POINTER(ctypes.c_uint), ctypes.c_uint]
    lib.emu_ellswift_schedule.restype = None
    lib.emu_ellswift_branch_value.argtypes = [cp, ctypes.c_uint]
    lib.emu_ellswift_midstate.argtypes = [cp]
    lib.emu_ellswift_midstate.restype = None
    return lib


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "ellswift_vectors.json")))


def _decode(emu, ell64, fmt):
    out = ctypes.create_string_buffer(b"\xaa" * OUT_BYTES[fmt], OUT_BYTES[fmt])
    emu.emu_ellswift_decode(out, fmt, ell64)
    return out.raw


def _encode(emu, key, fmt, rnd, cap=E.MAX_ATTEMPTS):
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64); capped = ctypes.c_int(7)
    r = emu.emu_ellswift_encode(out, ctypes.byref(capped), key, fmt, rnd, cap)
    return r, out.raw, capped.value


def test_golden_file_has_what_the_tests_need(golden):
    assert len(golden["xswiftec_inv"]) >= 30 and len(golden["decode"]) >= 100 and len(golden["encode"]) == 64 and len(golden["refused"]) == 6
    names = [r[0] for r in golden["decode"]]
    for u in ("0", "p", "p+1", "2^256-1"):
        for t in ("0", "p", "p+1", "2^256-1"):
            assert "u=%s t=%s" % (u, t) in names
    assert "g+s=0" in names and any("odd" in n for n in names) and any("even" in n for n in names)
    for which in (1, 2, 3):
        assert sum(1 for r in golden["decode"] if r[3] == which) >= 4
    att = [r[5] for r in golden["encode"]]
    assert set(r[6] for r in golden["encode"]) == set(range(8)) and min(att) == 1 and max(att) >= 12
    assert {r[0] for r in golden["refused"]} >= {"prefix 04", "prefix 05", "x = p", "x off the curve", "all-zero object"}


def test_model_against_the_golden_file(golden):
    for u, x, bitmap, encs in golden["xswiftec_inv"]:
        u, x = int(u, 16), int(x, 16)
        for c in range(8):
            t = E.xswiftec_inv(x, u, c)
            assert (t is not None) == bool((bitmap >> c) & 1)
            if t is not None:
                assert t == int(encs[c], 16) and E.xswiftec(u, t)[0] == x
    for name, ell, obj, which in golden["decode"]:
        x, y, w = E.decode(bytes.fromhex(ell))
        assert E.pubkey_object(x, y).hex() == obj and w == which, name
    for name, key33, obj, rnd, ell, att, c in golden["encode"]:
        assert E.encode(bytes.fromhex(key33), 2, bytes.fromhex(rnd)) == (1, bytes.fromhex(ell), att, c), name
        assert E.encode(bytes.fromhex(obj), 1, bytes.fromhex(rnd))[1].hex() == ell, name
        assert E.decode_out(bytes.fromhex(ell), 1).hex() == obj, name
    for name, key, fmt in golden["refused"]:
        assert E.encode(bytes.fromhex(key), fmt, bytes(32))[:2] == (0, bytes(64)), name
    g = E.decode_edges()
    assert E.g_plus_s_zero(int.from_bytes(dict(g)["g+s=0"][:32], "big"), int.from_bytes(dict(g)["g+s=0"][32:], "big"))


def test_midstate_is_the_tagged_hash_prefix(emu):
    out = ctypes.create_string_buffer(32)
    emu.emu_ellswift_midstate(out)
    from tests import s2c_ref
    want = s2c_ref.tag_midstate(b"secp256k1_ellswift_encode")            # a compression from the initial state, written out in Python
    assert out.raw == b"".join(w.to_bytes(4, "big") for w in want)
    th = hashlib.sha256(b"secp256k1_ellswift_encode").digest()
    assert E.tag_prefix() == th + th


def test_decode_every_golden_item_in_every_format(emu, golden):
    for name, ell, obj, which in golden["decode"] + [[r[0], r[4], r[2], None] for r in golden["encode"]]:
        ell, obj = bytes.fromhex(ell), bytes.fromhex(obj)
        x, y = int.from_bytes(obj[:32], "little"), int.from_bytes(obj[32:], "little")
        assert _decode(emu, ell, 1) == obj, name
        assert _decode(emu, ell, 0) == x.to_bytes(32, "big"), name
        assert _decode(emu, ell, 2) == E.ser33(x, y), name
        if which is not None:
            assert emu.emu_ellswift_which(ell, 3) == which and emu.emu_ellswift_which(ell, 2) == which, name


def test_partial_inverse_vectors_all_c(emu, golden):
    ran = 0
    for u, x, bitmap, encs in golden["xswiftec_inv"]:
        ub, xb = bytes.fromhex(u), bytes.fromhex(x)
        for c in range(8):
            t32 = ctypes.create_string_buffer(32)
            ok = emu.emu_ellswift_inv(t32, xb, ub, c)
            assert ok == ((bitmap >> c) & 1), (u, c)
            if ok:
                assert t32.raw.hex() == encs[c], (u, c)
                assert _decode(emu, ub + t32.raw, 0) == xb, (u, c)
                ran += 1
    assert ran == sum(bin(r[2]).count("1") for r in golden["xswiftec_inv"]) and ran > 0


def test_partial_inverse_against_the_model_on_seeded_pairs(emu):
    import random
    rng = random.Random(99)
    pt = E.pt_mul(12345, E.G)
    hits = 0
    for _ in range(48):
        u = rng.randrange(1, E.P)
        for c in range(8):
            t32 = ctypes.create_string_buffer(32)
            ok = emu.emu_ellswift_inv(t32, pt[0].to_bytes(32, "big"), u.to_bytes(32, "big"), c)
            want = E.xswiftec_inv(pt[0], u, c)
            assert bool(ok) == (want is not None) and (not ok or int.from_bytes(t32.raw, "big") == want), (u, c)
            hits += ok
    assert 48 < hits < 48 * 4                               # about one c in four succeeds


def test_counter_and_branch_helpers_past_the_first_pool(emu):
    pool = hashlib.sha256(b"pool").digest()
    for a in range(201):
        out = (ctypes.c_uint * 4)()
        emu.emu_ellswift_schedule(out, a)
        b, sh = E.branch_index(a)
        assert list(out) == [E.pool_counter(a), E.draw_counter(a), b, sh], a
        assert emu.emu_ellswift_branch_value(pool, a) == E.branch_value(pool, a), a
    # the reference's loop written out: counters in the order it consumes them
    cnt, left, order = 0, 0, []
    for a in range(201):
        if left == 0:
            order.append(("pool", cnt)); cnt += 1; left = 64
        left -= 1
        order.append(("u", cnt, left >> 1, (left & 1) << 2)); cnt += 1
    us = [o for o in order if o[0] == "u"]
    assert [(o[1], o[2], o[3]) for o in us] == [(E.draw_counter(a),) + E.branch_index(a) for a in range(201)]
    assert [o[1] for o in order if o[0] == "pool"] == sorted({E.pool_counter(a) for a in range(201)})


def test_encode_golden_items_byte_for_byte(emu, golden):
    for name, key33, obj, rnd, ell, att, c in golden["encode"]:
        for key, fmt in ((bytes.fromhex(obj), 1), (bytes.fromhex(key33), 2)):
            assert _encode(emu, key, fmt, bytes.fromhex(rnd)) == (1, bytes.fromhex(ell), 0), (name, fmt)


def test_encode_refused_keys(emu, golden):
    for name, key, fmt in golden["refused"]:
        assert _encode(emu, bytes.fromhex(key), fmt, bytes(32)) == (0, bytes(64), 0), name


def test_encode_attempt_cap(emu, golden):
    """an item cut off below its attempt count: 0, zero bytes and the capped flag; at its count: the reference's bytes"""
    row = max(golden["encode"], key=lambda r: r[5])
    key, rnd, att = bytes.fromhex(row[1]), bytes.fromhex(row[3]), row[5]
    assert att >= 12
    assert _encode(emu, key, 2, rnd, att - 1) == (0, bytes(64), 1)
    assert _encode(emu, key, 2, rnd, att) == (1, bytes.fromhex(row[4]), 0)
    assert E.encode(key, 2, rnd, att - 1)[:2] == (0, bytes(64))


def test_lane_routines_fit_their_buffers_under_the_sanitizers(golden, tmp_path):
    """tests/host_emul/ellswift_bounds (its own main, -fsanitize=address,undefined, runtimes linked statically): decode and encode over the
    golden items with every buffer of exactly its documented size on the heap"""
    prog = os.path.join(HERE, "host_emul", "ellswift_bounds")
    assert os.path.exists(prog), "tests/host_emul/ellswift_bounds not built (python -c 'import __graft_entry__ as g; g.build()')"
    dec = [(bytes.fromhex(r[1]), bytes.fromhex(r[2])) for r in golden["decode"]]
    enc = golden["encode"][:16] + [max(golden["encode"], key=lambda r: r[5])]
    blob = struct.pack("<III", len(dec), len(enc), len(golden["refused"]))
    blob += b"".join(a + b for a, b in dec)
    blob += b"".join(bytes.fromhex(r[1]) + bytes.fromhex(r[2]) + bytes.fromhex(r[3]) + bytes.fromhex(r[4]) for r in enc)
    blob += b"".join(bytes([fmt]) + bytes.fromhex(key).ljust(64, b"\0") for _, key, fmt in golden["refused"])
    path = tmp_path / "items.bin"
    path.write_bytes(blob)
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d %d %d" % (len(dec), len(enc), len(golden["refused"])) and "ERROR" not in r.stderr \
        and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, api, build_lib
    assert "engine_ellswift" in build_lib.UNITS_ADDED and build_lib.UNITS_ADDED[-1] == "engine_musig_agg"
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in ELLSWIFT_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "src/modules/ellswift/main_impl.h:470-483" in hdr and "src/modules/ellswift/main_impl.h:393-420" in hdr
    assert "#define S2K_OPT_ELLSWIFT_MAX_ATTEMPTS 14" in hdr and api.Engine.OPT_ELLSWIFT_MAX_ATTEMPTS == 14
    for m in ("ellswift_decode", "ellswift_decode_dev", "ellswift_encode", "ellswift_encode_dev", "ellswift_capped"):
        assert hasattr(api.Engine, m), m
    assert hasattr(api.Group, "ellswift_decode")


def test_library_exports_ellswift():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in ELLSWIFT_SYMBOLS:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ELLSWIFT_SYMBOLS:
        assert (" T " + name + "\n") in out, name
    # NULL engine / group: the call fails with a message, whatever the device situation
    assert lib.secp256k1_ellswift_decode_batch(None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ellswift_decode_batch_dev(None, None, None, 0, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ellswift_encode_batch(None, None, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ellswift_encode_batch_dev(None, None, None, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_ellswift_decode_batch_group(None, None, 0, None, 1) == 0 and "null group" in _native.last_error()
    # the single-item forms check their arguments before they look for a device
    lib.s2k_clear_status()
    assert lib.secp256k1_ellswift_decode_amd(None, None, None) == 0 and lib.s2k_last_status() == 2
    lib.s2k_clear_status()
    assert lib.secp256k1_ellswift_encode_amd(None, None, None, None) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    from secp256k1_zkp_amd import api
    with pytest.raises(ValueError):
        api._ellswift_decode_args("t", bytes(63), 1)
    with pytest.raises(ValueError):
        api._ellswift_decode_args("t", bytes(64), 3)
    with pytest.raises(ValueError):
        api._ellswift_encode_args("t", bytes(33), 0, bytes(32))
    with pytest.raises(ValueError):
        api._ellswift_encode_args("t", bytes(33), 2, bytes(31))
    assert api._ellswift_decode_args("t", bytes(128), 2)[1] == 2 and api._ellswift_encode_args("t", bytes(66), 2, bytes(64))[2] == 2


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_ellswift_decode_batch(0, 0, 0, 0, 0) + '
                   'secp256k1_ellswift_encode_batch(0, 0, 0, 0, 0, 0, 0) + secp256k1_ellswift_decode_amd(0, 0, 0) + secp256k1_ellswift_encode_amd(0, 0, 0, 0) + '
                   '(int)s2k_engine_ellswift_capped(0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "ellswift_decode.c"), "-o", str(tmp_path / "e.o")], check=True)
