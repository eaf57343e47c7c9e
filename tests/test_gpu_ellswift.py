"""GPU: ElligatorSwift decoding and encoding (csrc/ellswift.h, csrc/engine_ellswift.hip) through the C ABI.  The answers are the
reference's own where they are recorded (tests/golden/ellswift_vectors.json) and the Python model's (tests/ellswift_ref.py, which agrees
with the reference on every recorded item) elsewhere.  Every comparison is exact."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import ellswift_ref as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT_BYTES = {0: 32, 1: 64, 2: 33}
KEY_BYTES = {1: 64, 2: 33}
SIZES = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "ellswift_vectors.json")))


@pytest.fixture(scope="module")
def dec_items(golden):
    """[(ell64, object)]: every recorded decode item, then every recorded encoding; never changed"""
    return [(bytes.fromhex(r[1]), bytes.fromhex(r[2])) for r in golden["decode"]] + [(bytes.fromhex(r[4]), bytes.fromhex(r[2])) for r in golden["encode"]]


@pytest.fixture(scope="module")
def enc_items(golden):
    """[(key33, object, rnd32, ell64, attempts)]"""
    return [(bytes.fromhex(r[1]), bytes.fromhex(r[2]), bytes.fromhex(r[3]), bytes.fromhex(r[4]), r[5]) for r in golden["encode"]]


def _arr(bs, w):
    return np.frombuffer(b"".join(bs), np.uint8).reshape(len(bs), w).copy()


def _want(obj, fmt):
    x, y = int.from_bytes(obj[:32], "little"), int.from_bytes(obj[32:], "little")
    return x.to_bytes(32, "big") if fmt == 0 else obj if fmt == 1 else E.ser33(x, y)


def _cycle(items, n, start=0):
    return [items[(start + i) % len(items)] for i in range(n)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _check_decode(obj, items, fmt, what):
    got = obj.ellswift_decode(_arr([x[0] for x in items], 64), out_format=fmt)
    want = _arr([_want(x[1], fmt) for x in items], OUT_BYTES[fmt])
    assert got.shape == want.shape and np.array_equal(got, want), (what, fmt, np.flatnonzero((got != want).any(axis=1))[:8])


def _check_encode(engine, items, fmt, what):
    res, got = engine.ellswift_encode(_arr([x[1] if fmt == 1 else x[0] for x in items], KEY_BYTES[fmt]), _arr([x[2] for x in items], 32), key_format=fmt)
    want = _arr([x[3] for x in items], 64)
    assert np.array_equal(res, np.ones(len(items), np.int32)) and np.array_equal(got, want), (what, fmt, np.flatnonzero((got != want).any(axis=1))[:8])


def test_decode_golden_vectors_three_formats(engine, dec_items):
    for fmt in (0, 1, 2):
        _check_decode(engine, dec_items, fmt, "golden")


def test_encode_golden_vectors_two_key_formats(engine, enc_items):
    for fmt in (1, 2):
        _check_encode(engine, enc_items, fmt, "golden")
    assert engine.ellswift_capped() == 0


def test_batch_sizes(engine, dec_items, enc_items):
    """1, 63, 64, 65 and 130 items cut cyclically from the recorded ones: the tail lanes of the last wavefront and the shared inversion"""
    for n in SIZES:
        for fmt in (0, 1, 2):
            _check_decode(engine, _cycle(dec_items, n, start=n), fmt, n)
        for fmt in (1, 2):
            _check_encode(engine, _cycle(enc_items, n, start=n), fmt, n)


def test_refused_key_in_the_middle_of_a_wavefront(engine, golden, enc_items):
    """every refused key at lane 31 of 64 valid items (and with a second wavefront behind): 0 and zero bytes for it, the reference's bytes
    for its 63 neighbours"""
    for name, key, fmt in golden["refused"]:
        key = bytes.fromhex(key)
        for n in (64, 130):
            items = _cycle(enc_items, n)
            keys = [x[1] if fmt == 1 else x[0] for x in items]; keys[31] = key
            res, got = engine.ellswift_encode(_arr(keys, KEY_BYTES[fmt]), _arr([x[2] for x in items], 32), key_format=fmt)
            want = _arr([x[3] for x in items], 64); want[31] = 0
            wres = np.ones(n, np.int32); wres[31] = 0
            assert np.array_equal(res, wres) and np.array_equal(got, want), (name, n)
    assert engine.ellswift_capped() == 0


def test_first_attempt_item_next_to_the_longest(engine, enc_items):
    """one wavefront that mixes items that succeed at once with the item that needs the most attempts (>= 12): the finished lanes wait
    with 1 in the shared inversion and keep their bytes"""
    first = [x for x in enc_items if x[4] == 1]
    longest = max(enc_items, key=lambda x: x[4])
    assert first and longest[4] >= 12
    items = [first[i % len(first)] for i in range(64)]
    for lane in (0, 17, 63):
        batch = list(items); batch[lane] = longest
        for fmt in (1, 2):
            _check_encode(engine, batch, fmt, lane)


def test_attempt_cap(enc_items, engine):
    """S2K_OPT_ELLSWIFT_MAX_ATTEMPTS below an item's attempt count: that item gets 0 and zero bytes and is counted, every item that needs
    no more attempts than the cap keeps the reference's bytes"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        cap = 3
        eng.set_option(Engine.OPT_ELLSWIFT_MAX_ATTEMPTS, cap)
        res, got = eng.ellswift_encode(_arr([x[0] for x in enc_items], 33), _arr([x[2] for x in enc_items], 32), key_format=2)
        wres = np.array([int(x[4] <= cap) for x in enc_items], np.int32)
        want = _arr([x[3] if x[4] <= cap else bytes(64) for x in enc_items], 64)
        assert 0 < wres.sum() < len(enc_items)
        assert np.array_equal(res, wres) and np.array_equal(got, want)
        assert eng.ellswift_capped() == len(enc_items) - int(wres.sum())
        with pytest.raises(RuntimeError):
            eng.set_option(Engine.OPT_ELLSWIFT_MAX_ATTEMPTS, 257)
        with pytest.raises(RuntimeError):
            eng.set_option(Engine.OPT_ELLSWIFT_MAX_ATTEMPTS, 0)
        eng.set_option(Engine.OPT_ELLSWIFT_MAX_ATTEMPTS, 256)
        _check_encode(eng, enc_items, 2, "cap lifted")
    finally:
        eng.close()


def test_dev_forms_zero_poisoned_outputs(engine, dec_items, enc_items):
    """the _dev forms on a caller's stream into outputs pre-filled with 0xA5 / 7; a refused key among the encode items must come out as zeros"""
    import torch
    s = torch.cuda.Stream()
    st = ctypes.c_void_p(s.cuda_stream)
    items = _cycle(dec_items, 130, start=5)
    d_in = _dev(_arr([x[0] for x in items], 64))
    for fmt in (0, 1, 2):
        d_out = torch.full((130, OUT_BYTES[fmt]), 0xA5, dtype=torch.uint8, device="cuda:0")
        s.wait_stream(torch.cuda.current_stream())
        engine.ellswift_decode_dev(d_out, d_in, out_format=fmt, stream=st)
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), _arr([_want(x[1], fmt) for x in items], OUT_BYTES[fmt])), fmt
    items = _cycle(enc_items, 65, start=2)
    for fmt in (1, 2):
        keys = [x[1] if fmt == 1 else x[0] for x in items]
        keys[40] = bytes(64) if fmt == 1 else b"\x04" + keys[40][1:]
        d_res = torch.full((65,), 7, dtype=torch.int32, device="cuda:0"); d_out = torch.full((65, 64), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_key, d_rnd = _dev(_arr(keys, KEY_BYTES[fmt])), _dev(_arr([x[2] for x in items], 32))
        s.wait_stream(torch.cuda.current_stream())
        engine.ellswift_encode_dev(d_res, d_out, d_key, d_rnd, key_format=fmt, stream=st)
        s.synchronize()
        want = _arr([x[3] for x in items], 64); want[40] = 0
        wres = np.ones(65, np.int32); wres[40] = 0
        assert np.array_equal(d_res.cpu().numpy(), wres) and np.array_equal(d_out.cpu().numpy(), want), fmt


def test_encode_then_decode_on_the_device(engine, enc_items):
    """keys -> encodings -> keys without leaving HBM, in both key formats"""
    import torch
    items = _cycle(enc_items, 130)
    for fmt in (1, 2):
        d_key = _dev(_arr([x[1] if fmt == 1 else x[0] for x in items], KEY_BYTES[fmt])); d_rnd = _dev(_arr([x[2] for x in items], 32))
        d_res = torch.zeros((130,), dtype=torch.int32, device="cuda:0"); d_ell = torch.zeros((130, 64), dtype=torch.uint8, device="cuda:0")
        d_back = torch.zeros((130, KEY_BYTES[fmt]), dtype=torch.uint8, device="cuda:0")
        engine.ellswift_encode_dev(d_res, d_ell, d_key, d_rnd, key_format=fmt)
        engine.ellswift_decode_dev(d_back, d_ell, out_format=fmt)
        engine.sync()
        assert d_res.cpu().numpy().all() and torch.equal(d_back, d_key), fmt


def test_decoded_keys_feed_the_ecdsa_verifier_and_tweak_add(engine, enc_items):
    """decode format 1 on the device straight into secp256k1_ecdsa_verify_batch_dev: the verdicts of the same keys passed directly (valid
    signatures, one in four with a flipped message bit); decode format 2 agrees with format 1 through secp256k1_pubkey_tweak_add_batch with
    a zero tweak"""
    import torch
    rng = random.Random(3240)
    secrets = E.encode_item_secrets(rng)
    n = 24
    items = enc_items[:n]
    msgs, sigs = [], []
    for i, it in enumerate(items):
        m = bytes(rng.randrange(256) for _ in range(32))
        sigs.append(E.ecdsa_sign(secrets[i % 8], m, rng.randrange(1, E.N)))
        msgs.append(m if i % 4 else bytes([m[0] ^ 1]) + m[1:])
    objs = _arr([x[1] for x in items], 64)
    direct = engine.ecdsa_verify_batch(_arr(sigs, 64), _arr(msgs, 32), objs, sig_format=0, pk_format=1)
    assert list(direct) == [int(i % 4 != 0) for i in range(n)]
    d_keys = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda:0"); d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    engine.ellswift_decode_dev(d_keys, _dev(_arr([x[3] for x in items], 64)), out_format=1)
    engine.ecdsa_verify_batch_dev(d_res, _dev(_arr(sigs, 64)), _dev(_arr(msgs, 32)), d_keys, sig_format=0, pk_format=1)
    engine.sync()
    assert np.array_equal(d_res.cpu().numpy(), direct) and np.array_equal(d_keys.cpu().numpy(), objs)
    ell = _arr([x[3] for x in items], 64)
    r1, k1 = engine.pubkey_tweak_add_batch(engine.ellswift_decode(ell, out_format=1), np.zeros((n, 32), np.uint8), key_format=1)
    r2, k2 = engine.pubkey_tweak_add_batch(engine.ellswift_decode(ell, out_format=2), np.zeros((n, 32), np.uint8), key_format=2)
    assert r1.all() and r2.all() and np.array_equal(k1, k2) and np.array_equal(k1, objs)


def test_amd_forms(engine, dec_items, enc_items, golden):
    L = engine._lib
    for ell, obj in dec_items[:6] + dec_items[-3:]:
        out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
        assert L.secp256k1_ellswift_decode_amd(None, out, ell) == 1 and L.s2k_last_status() == 0 and out.raw == obj
    for key33, obj, rnd, ell, att in enc_items[:4]:
        out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
        assert L.secp256k1_ellswift_encode_amd(None, out, obj, rnd) == 1 and L.s2k_last_status() == 0 and out.raw == ell
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    assert L.secp256k1_ellswift_encode_amd(None, out, bytes(64), bytes(32)) == 0 and L.s2k_last_status() == 0 and out.raw == bytes(64)
    assert L.secp256k1_ellswift_decode_amd(None, out, None) == 0 and L.s2k_last_status() == 2 and out.raw == bytes(64)
    assert L.secp256k1_ellswift_encode_amd(None, out, None, bytes(32)) == 0 and L.s2k_last_status() == 2


def test_batch_argument_checks(engine, dec_items, enc_items):
    """NULL where the reference has ARG_CHECK and a format out of range fail the call with the argument status; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    ell = _arr([x[0] for x in dec_items[:4]], 64); out = np.full((4, 64), 7, np.uint8)
    assert L.secp256k1_ellswift_decode_batch(h, p(out), 1, p(ell), 4) == 1 and np.array_equal(out, _arr([x[1] for x in dec_items[:4]], 64))
    for args in ((None, 1, p(ell), 4), (p(out), 1, None, 4), (p(out), 3, p(ell), 4), (p(out), -1, p(ell), 4)):
        assert L.secp256k1_ellswift_decode_batch(h, *args) == 0 and L.s2k_last_status() == 2, args
        assert L.secp256k1_ellswift_decode_batch_dev(h, None, *args) == 0 and L.s2k_last_status() == 2, args
        assert L.secp256k1_ellswift_decode_batch_group(None, *args) == 0
    keys = _arr([x[0] for x in enc_items[:4]], 33); rnd = _arr([x[2] for x in enc_items[:4]], 32); res = np.full(4, 7, np.int32)
    good = [p(res), p(out), p(keys), 2, p(rnd), 4]
    assert L.secp256k1_ellswift_encode_batch(h, *good) == 1 and res.all() and np.array_equal(out, _arr([x[3] for x in enc_items[:4]], 64))
    for k, bad in ((0, None), (1, None), (2, None), (4, None), (3, 0), (3, 3)):
        b = list(good); b[k] = bad
        assert L.secp256k1_ellswift_encode_batch(h, *b) == 0 and L.s2k_last_status() == 2, (k, bad)
        assert L.secp256k1_ellswift_encode_batch_dev(h, None, *b) == 0 and L.s2k_last_status() == 2, (k, bad)
    assert L.secp256k1_ellswift_decode_batch(h, None, 1, None, 0) == 1 and L.secp256k1_ellswift_decode_batch_dev(h, None, None, 1, None, 0) == 1
    assert L.secp256k1_ellswift_encode_batch(h, None, None, None, 1, None, 0) == 1 and L.secp256k1_ellswift_encode_batch_dev(h, None, None, None, None, 1, None, 0) == 1
    assert engine.ellswift_decode(b"").shape == (0, 64) and engine.ellswift_encode(b"", b"")[0].size == 0


def test_group_form_two_engines_of_device_0(dec_items):
    from secp256k1_zkp_amd import Group
    g = Group([0, 0])
    try:
        assert len(g) == 2
        for n in (1, 65, 130):
            for fmt in (0, 1, 2):
                _check_decode(g, _cycle(dec_items, n, start=7), fmt, ("group", n))
    finally:
        g.close()


def test_sub_range_launches(dec_items, enc_items):
    """600 items on an engine whose launches take 256 lanes: the second and third launch start at the right item"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        for fmt in (0, 1, 2):
            _check_decode(eng, _cycle(dec_items, 600), fmt, "sub-range")
        for fmt in (1, 2):
            _check_encode(eng, _cycle(enc_items, 600), fmt, "sub-range")
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_c_example(tmp_path, dec_items, enc_items):
    """examples/ellswift_decode.c (gcc -std=c99) linked against the shared library: decode, encode again, decode back"""
    exe = str(tmp_path / "ellswift_decode")
    libdir = os.path.join(ROOT, "secp256k1_zkp_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ellswift_decode.c"), "-o", exe,
                    os.path.join(libdir, "libsecp256k1_zkp_amd.so"), "-Wl,-rpath," + libdir], check=True)
    items = dec_items[:70]
    (tmp_path / "items.bin").write_bytes(b"".join(x[0] + enc_items[i % len(enc_items)][2] for i, x in enumerate(items)))
    out = subprocess.run([exe, str(tmp_path / "items.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr)
    lines = out.stdout.strip().split("\n")
    assert lines[:-1] == [_want(x[1], 2).hex() for x in items] and lines[-1] == "round trip: 0 keys lost"


def test_lane_routines_on_the_device(golden):
    """tests/gpu_prims/ellswift_prims.hip: the partial inverse for all eight c on the module's vectors (253 lanes: three wavefronts and a partial
    one, refused lanes next to accepted ones), the candidate the fraction routine takes, and the counter / branch helpers for
    attempts 0..200"""
    import hashlib
    import torch
    path = os.path.join(HERE, "gpu_prims", "libs2k_ellswift_prims.so")
    assert os.path.exists(path), "tests/gpu_prims/libs2k_ellswift_prims.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.s2k_test_ellswift_inv.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int]
    L.s2k_test_ellswift_which.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2
    L.s2k_test_ellswift_schedule.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int]
    xs, us, cs, want_ok, want_t = [], [], [], [], []
    for u, x, bitmap, encs in golden["xswiftec_inv"]:
        for c in range(8):
            xs.append(bytes.fromhex(x)); us.append(bytes.fromhex(u)); cs.append(c)
            want_ok.append((bitmap >> c) & 1); want_t.append(bytes.fromhex(encs[c]))
    n = len(cs) - 3                                                                       # (253 lanes: the last wavefront is a partial one)
    xs, us, cs, want_ok, want_t = xs[:n], us[:n], cs[:n], want_ok[:n], want_t[:n]
    assert n % 64 != 0 and n > 128
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_t = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    d_x, d_u, d_c = _dev(_arr(xs, 32)), _dev(_arr(us, 32)), _dev(np.array(cs, np.int32))
    torch.cuda.synchronize()
    assert L.s2k_test_ellswift_inv(d_ok.data_ptr(), d_t.data_ptr(), d_x.data_ptr(), d_u.data_ptr(), d_c.data_ptr(), n) == 1
    ok = d_ok.cpu().numpy(); t = d_t.cpu().numpy()
    assert list(ok) == want_ok
    assert all(t[i].tobytes() == want_t[i] for i in range(n) if want_ok[i])
    dec = golden["decode"]
    d_w = torch.zeros((len(dec),), dtype=torch.int32, device="cuda:0"); d_e = _dev(_arr([bytes.fromhex(r[1]) for r in dec], 64))
    for roots in (2, 3):
        assert L.s2k_test_ellswift_which(d_w.data_ptr(), d_e.data_ptr(), roots, len(dec)) == 1
        assert list(d_w.cpu().numpy()) == [r[3] for r in dec], roots
    pool = hashlib.sha256(b"pool").digest()
    d_s = torch.zeros((201, 5), dtype=torch.int32, device="cuda:0")
    assert L.s2k_test_ellswift_schedule(d_s.data_ptr(), _dev(np.frombuffer(pool, np.uint8).copy()).data_ptr(), 201) == 1
    got = d_s.cpu().numpy()
    assert [list(r) for r in got] == [[E.pool_counter(a), E.draw_counter(a), E.branch_index(a)[0], E.branch_index(a)[1], E.branch_value(pool, a)] for a in range(201)]
