"""GPU: Taproot tweak checks and public-key tweak-add (csrc/tweak.h, csrc/engine_tweak.hip) against the unmodified reference
(oracle/_ref through tests/tweak_ref.py): every verdict and every output key is the reference's, asked in this run."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY_BYTES = {0: 32, 1: 64, 2: 33}


@pytest.fixture(scope="module")
def tref(ref):
    from tests.tweak_ref import TweakRef
    return TweakRef()


@pytest.fixture(scope="module")
def edge(tref):
    from tests.tweak_ref import edge_cases
    return edge_cases(tref)


@pytest.fixture(scope="module")
def rnd(tref):
    """600 seeded items, every fourth one corrupted, both key formats; shared by the tests below and never changed"""
    from tests.tweak_ref import random_items
    items = random_items(tref, 600, 4404)
    ones = sum(x[6] for x in items)
    assert ones >= 75 and 600 - ones >= 75
    return items


def _arr(items, col, width):
    return np.frombuffer(b"".join(x[col] for x in items), np.uint8).reshape(len(items), width).copy()


def _check_arrays(items):
    """items of ONE key_format -> (tweaked32, parities, keys, tweaks32, expected verdicts)"""
    fmt = items[0][1]
    assert all(x[1] == fmt and x[6] is not None for x in items)
    return (_arr(items, 4, 32), np.array([x[5] for x in items], np.uint8), _arr(items, 2, KEY_BYTES[fmt]), _arr(items, 3, 32),
            np.array([x[6] for x in items], np.int32))


def _add_arrays(items):
    """items of ONE key_format -> (keys, tweaks32, expected verdicts, expected output objects)"""
    fmt = items[0][1]
    assert all(x[1] == fmt and x[7] is not None for x in items)
    return _arr(items, 2, KEY_BYTES[fmt]), _arr(items, 3, 32), np.array([x[7] for x in items], np.int32), _arr(items, 8, 64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _names(items, got, exp):
    return [x[0] for x, g, e in zip(items, got, exp) if g != e]


def _check_dev(engine, tw, par, keys, t, fmt):
    import torch
    d_res = torch.full((len(par),), 7, dtype=torch.int32, device="cuda:0")
    engine.xonly_tweak_add_check_batch_dev(d_res, _dev(tw), _dev(par), _dev(keys), _dev(t), key_format=fmt)
    engine.sync()
    return d_res.cpu().numpy()


def _add_dev(engine, keys, t, fmt):
    import torch
    n = t.shape[0]
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_out = torch.full((n, 64), 0xFF, dtype=torch.uint8, device="cuda:0")
    engine.pubkey_tweak_add_batch_dev(d_res, d_out, _dev(keys), _dev(t), key_format=fmt)
    engine.sync()
    return d_res.cpu().numpy(), d_out.cpu().numpy()


def test_edge_list_host_dev_group(engine, edge):
    """the edge list, format by format, through the host, _dev and group forms; _dev writes into results pre-filled with 7 and an output
    tensor pre-filled with 0xFF: refused items read 0 and 64 zero bytes"""
    import torch
    from secp256k1_zkp_amd import Group
    g = Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0])
    try:
        for fmt in (0, 1):
            items = [x for x in edge if x[1] == fmt and x[6] is not None]
            tw, par, keys, t, exp = _check_arrays(items)
            assert 0 < exp.sum() < len(items)
            got = engine.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt)
            assert np.array_equal(got, exp), _names(items, got, exp)
            got = _check_dev(engine, tw, par, keys, t, fmt)
            assert np.array_equal(got, exp), _names(items, got, exp)
            got = g.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt)
            assert np.array_equal(got, exp), _names(items, got, exp)
            for k in (1, 2, 3):
                assert np.array_equal(g.xonly_tweak_add_check_batch(tw[:k], par[:k], keys[:k], t[:k], key_format=fmt), exp[:k])
        for fmt in (0, 1, 2):
            items = [x for x in edge if x[1] == fmt and x[7] is not None]
            keys, t, exp, eout = _add_arrays(items)
            assert 0 < exp.sum() < len(items) and not eout[exp == 0].any()
            got, out = engine.pubkey_tweak_add_batch(keys, t, key_format=fmt)
            assert np.array_equal(got, exp), _names(items, got, exp)
            assert np.array_equal(out, eout), _names(items, out.tolist(), eout.tolist())
            got, out = _add_dev(engine, keys, t, fmt)
            assert np.array_equal(got, exp) and np.array_equal(out, eout), _names(items, got, exp)
    finally:
        g.close()


def test_single_item_forms(engine, edge, tref):
    """the three _amd forms on the edge list's key objects, with the reference's argument lists"""
    L = engine._lib
    items = [x for x in edge if x[1] == 1]
    assert {x[5] for x in items} >= {0, 1, 2, 255}
    for name, fmt, key, t, tw, par, cv, av, out in items:
        assert L.secp256k1_xonly_pubkey_tweak_add_check_amd(None, tw, par, key, t) == cv and L.s2k_last_status() == 0, name
        if av is None:
            continue
        o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_xonly_pubkey_tweak_add_amd(None, o, key, t) == av and o.raw == out and L.s2k_last_status() == 0, name
        io = ctypes.create_string_buffer(key, 64)
        assert L.secp256k1_ec_pubkey_tweak_add_amd(None, io, t) == av and io.raw == out and L.s2k_last_status() == 0, name
    # a parity that is no byte: the reference compares the int
    name, fmt, key, t, tw, par, cv, av, out = next(x for x in items if x[6] == 1)
    for p in (-1, 256 + par, 1 << 20):
        assert L.secp256k1_xonly_pubkey_tweak_add_check_amd(None, tw, p, key, t) == 0 == tref.xonly_tweak_add_check(tw, p, key, t)
    # NULL where the reference has ARG_CHECK
    o = ctypes.create_string_buffer(64)
    for args in ((None, None, par, key, t), (None, tw, par, None, t), (None, tw, par, key, None)):
        assert L.secp256k1_xonly_pubkey_tweak_add_check_amd(*args) == 0 and L.s2k_last_status() == 2
    for args in ((None, None, key, t), (None, o, None, t), (None, o, key, None)):
        assert L.secp256k1_xonly_pubkey_tweak_add_amd(*args) == 0 and L.s2k_last_status() == 2
    for args in ((None, None, t), (None, o, None)):
        assert L.secp256k1_ec_pubkey_tweak_add_amd(*args) == 0 and L.s2k_last_status() == 2


def test_batch_argument_checks(engine, edge):
    """NULL arrays and a key_format out of range fail the call with the argument status; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    items = [x for x in edge if x[1] == 1 and x[6] is not None][:4]
    tw, par, keys, t, exp = _check_arrays(items)
    res = np.full(4, 7, np.int32); out = np.full((4, 64), 0xFF, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(tw), p(par), p(keys), 1, p(t), 4]
    assert L.secp256k1_xonly_pubkey_tweak_add_check_batch(h, *good) == 1 and np.array_equal(res, exp)
    for k in (0, 1, 2, 3, 5):
        a = list(good); a[k] = None
        assert L.secp256k1_xonly_pubkey_tweak_add_check_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
    for fmt in (2, 3, -1):                                # the check form takes no compressed keys
        a = list(good); a[4] = fmt
        assert L.secp256k1_xonly_pubkey_tweak_add_check_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any(), fmt
        assert L.secp256k1_xonly_pubkey_tweak_add_check_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, fmt
    a = list(good); a[6] = 0
    assert L.secp256k1_xonly_pubkey_tweak_add_check_batch(h, *a) == 1
    assert L.secp256k1_xonly_pubkey_tweak_add_check_batch(h, None, None, None, None, 0, None, 0) == 1
    good = [p(res), p(out), p(keys), 1, p(t), 4]
    for k in (0, 1, 2, 4):
        a = list(good); a[k] = None
        assert L.secp256k1_pubkey_tweak_add_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
    for fmt in (3, -1):
        a = list(good); a[3] = fmt
        assert L.secp256k1_pubkey_tweak_add_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not out.any(), fmt
        assert L.secp256k1_pubkey_tweak_add_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, fmt
    assert L.secp256k1_pubkey_tweak_add_batch(h, None, None, None, 0, None, 0) == 1
    assert engine.xonly_tweak_add_check_batch(b"", b"", b"", b"").size == 0


def _interleaved(valid, bad, n, dead_wave=None):
    """n items: every third one (i % 3 == 1) refused or with an infinite result, the others valid; dead_wave: a whole wavefront of them"""
    out = []
    for i in range(n):
        dead = i % 3 == 1 or (dead_wave is not None and 64 * dead_wave <= i < 64 * (dead_wave + 1))
        out.append(bad[i % len(bad)] if dead else valid[i % len(valid)])
    return out


def test_batch_sizes(engine, edge, rnd):
    """1, 63, 64, 65 and 257 items; refused and infinite-result items next to valid ones in every wavefront (the shared inversion sees
    lanes handing in z = 1 beside live ones), one batch with a whole wavefront of them, and the dead lanes of a partial last wavefront"""
    for fmt in (0, 1):
        valid = [x for x in rnd if x[1] == fmt and x[6] == 1 and x[7] == 1]
        bad = [x for x in edge if x[1] == fmt and x[7] == 0 and x[6] == 0]
        assert len(valid) >= 100 and len(bad) >= 6
        assert any("t = " in x[0] for x in bad) and any("tweak n" in x[0] for x in bad)       # infinite results and refused tweaks
        for n, dead_wave in ((1, None), (63, None), (64, None), (65, None), (257, None), (257, 1)):
            items = _interleaved(valid, bad, n, dead_wave)
            tw, par, keys, t, exp = _check_arrays(items)
            assert n < 3 or 0 < exp.sum() < n
            got = engine.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt)
            assert np.array_equal(got, exp), (fmt, n, dead_wave, np.flatnonzero(got != exp)[:8])
            keys, t, exp, eout = _add_arrays(items)
            got, out = engine.pubkey_tweak_add_batch(keys, t, key_format=fmt)
            assert np.array_equal(got, exp) and np.array_equal(out, eout), (fmt, n, dead_wave)
    # a lone refused item, and a lone item on the all-zero object
    for x in (bad[0], next(x for x in edge if x[0] == "fmt 1 all-zero object")):
        tw, par, keys, t, exp = _check_arrays([x])
        assert engine.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=1).tolist() == [0]
        got, out = engine.pubkey_tweak_add_batch(keys, t, key_format=1)
        assert got.tolist() == [0] and not out.any()


def test_sub_range_launches(engine, rnd):
    """600 items on an engine whose launches take 256 lanes: three sub-range launches, equal to the single-launch results"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        for fmt in (0, 1):
            items = [x for x in rnd if x[1] == fmt] * 2                   # 600 items of one format
            assert len(items) == 600
            tw, par, keys, t, exp = _check_arrays(items)
            one = engine.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt)
            assert np.array_equal(one, exp) and 0 < exp.sum() < 600
            assert np.array_equal(eng.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt), one)
            assert np.array_equal(_check_dev(eng, tw, par, keys, t, fmt), one)
            keys, t, exp, eout = _add_arrays(items)
            one, out1 = engine.pubkey_tweak_add_batch(keys, t, key_format=fmt)
            assert np.array_equal(one, exp) and np.array_equal(out1, eout)
            got, out = eng.pubkey_tweak_add_batch(keys, t, key_format=fmt)
            assert np.array_equal(got, one) and np.array_equal(out, out1)
            got, out = _add_dev(eng, keys, t, fmt)
            assert np.array_equal(got, one) and np.array_equal(out, out1)
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_table_widths(engine, rnd, edge):
    """300 random items and the recoding-boundary items at a 20-bit generator table and again at the default width"""
    from secp256k1_zkp_amd import Engine
    items = rnd[:300] + [x for x in edge if x[0].startswith("recoding ")]
    by_fmt = {fmt: [x for x in items if x[1] == fmt] for fmt in (0, 1)}
    try:
        for bits in (20, 26):
            engine.set_option(Engine.OPT_GTAB_BITS, bits)
            for fmt in (0, 1):
                tw, par, keys, t, exp = _check_arrays(by_fmt[fmt])
                got = engine.xonly_tweak_add_check_batch(tw, par, keys, t, key_format=fmt)
                assert int(engine._lib.s2k_engine_gtable_bits(engine._h)) == bits
                assert np.array_equal(got, exp), (bits, _names(by_fmt[fmt], got, exp))
                keys, t, exp, eout = _add_arrays(by_fmt[fmt])
                got, out = engine.pubkey_tweak_add_batch(keys, t, key_format=fmt)
                assert np.array_equal(got, exp) and np.array_equal(out, eout), (bits, _names(by_fmt[fmt], got, exp))
    finally:
        engine.set_option(Engine.OPT_GTAB_BITS, 26)


def test_add_output_feeds_the_check(engine, rnd, tref):
    """the add form's output objects, handed back as key_format 1 with tweak 0 and with a fresh tweak: the check form accepts the x and
    parity the reference derives from them"""
    from tests.tweak_ref import obj_x32, obj_parity
    items = [x for x in rnd if x[7] == 1][:200]
    keys, t, exp, eout = _add_arrays([x for x in items if x[1] == 1])
    got, out = engine.pubkey_tweak_add_batch(keys, t, key_format=1)
    assert got.all() and np.array_equal(out, eout)
    n = out.shape[0]
    # the outputs as internal keys (objects with either parity of y, as they are) under a second tweak
    t2 = np.roll(t, 1, axis=0)
    second = [tref.add(1, out[i].tobytes(), t2[i].tobytes()) for i in range(n)]
    assert all(v for v, _ in second)
    tw = np.frombuffer(b"".join(obj_x32(o) for _, o in second), np.uint8).reshape(n, 32)
    par = np.array([obj_parity(o) for _, o in second], np.uint8)
    assert {0, 1} == set(par.tolist()) and {0, 1} == {int(o[32]) & 1 for o in out}
    exp = np.array([tref.check(1, out[i].tobytes(), tw[i].tobytes(), int(par[i]), t2[i].tobytes()) for i in range(n)], np.int32)
    assert exp.all()
    assert engine.xonly_tweak_add_check_batch(tw, par, out, t2, key_format=1).all()
    # and with tweak 0: the object's own x and parity
    tw0 = np.frombuffer(b"".join(obj_x32(out[i].tobytes()) for i in range(n)), np.uint8).reshape(n, 32)
    par0 = np.array([int(o[32]) & 1 for o in out], np.uint8)
    assert engine.xonly_tweak_add_check_batch(tw0, par0, out, np.zeros((n, 32), np.uint8), key_format=1).all()
