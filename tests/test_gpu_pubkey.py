"""GPU: public-key conversion, negation, tweak-mul and combine (csrc/pubkey.h, csrc/engine_pubkey.hip) against the unmodified reference
(oracle/_ref through tests/pubkey_ref.py): every verdict, every output byte and every parity is the reference's, asked in this run, and
compared item by item.  The engine's documented differences (the all-zero object, the empty set, a set with a key that does not load:
0 and zero bytes) carry the contract of tests/pubkey_ref.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PK_BYTES = {0: 32, 1: 64, 2: 33, 3: 65, 4: 64, 5: 64}
F = 16                  # the first pass's default chunk length (PUBKEY_FOLD_FANIN_DEFAULT)


@pytest.fixture(scope="module")
def pref(ref):
    from tests.pubkey_ref import PubkeyRef
    return PubkeyRef()


@pytest.fixture(scope="module")
def edge(pref):
    from tests.pubkey_ref import edge_cases, FANIN
    assert FANIN == F
    return edge_cases(pref)


@pytest.fixture(scope="module")
def rnd(pref):
    """300 seeded items per call, every fourth one corrupted; shared by the tests below and never changed"""
    from tests.pubkey_ref import random_items
    return random_items(pref, 300, 7706)


@pytest.fixture(scope="module")
def eng512():
    """an engine whose launches take 512 lanes, so that 1 100 items are three sub-range launches"""
    from secp256k1_zkp_amd import Engine
    e = Engine(0)
    e.set_option(Engine.OPT_MAX_LANES, 512)
    yield e
    e.close()


def _arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _fill(n, ob):
    """_dev outputs pre-filled with 7 / 0xFF: a refused item must read 0 and zero bytes afterwards"""
    import torch
    return (torch.full((n,), 7, dtype=torch.int32, device="cuda:0"), torch.full((n, ob), 0xFF, dtype=torch.uint8, device="cuda:0"),
            torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda:0"))


def _bad(items, got, exp):
    return [x[0] for x, g, e in zip(items, got, exp) if not np.array_equal(g, e)][:6]


def _cycle(items, n):
    return [items[i % len(items)] for i in range(n)]


# ---- convert and negate -----------------------------------------------------------------------------------------------------------------------
def _conv_expect(items, of, neg):
    oc, pc = (6, 7) if neg else (4, 5)
    return (np.array([x[3] for x in items], np.int32), _arr([x[oc][of] for x in items], PK_BYTES[of]), np.array([x[pc] for x in items], np.uint8))


def _conv_check(engine, items, fmt, of, neg, dev=False):
    keys = _arr([x[2] for x in items], PK_BYTES[fmt]); n = len(items)
    er, eo, ep = _conv_expect(items, of, neg)
    if dev:
        d_res, d_out, d_par = _fill(n, PK_BYTES[of])
        (engine.pubkey_negate_dev if neg else engine.pubkey_convert_dev)(d_res, d_out, _dev(keys), fmt, of, parities_out=d_par)
        engine.sync()
        res, out, par = d_res.cpu().numpy(), d_out.cpu().numpy(), d_par.cpu().numpy()
    else:
        res, out, par = (engine.pubkey_negate if neg else engine.pubkey_convert)(keys, fmt, of)
    assert np.array_equal(res, er), (fmt, of, neg, dev, _bad(items, res, er))
    assert np.array_equal(out, eo), (fmt, of, neg, dev, _bad(items, out, eo))
    assert np.array_equal(par, ep), (fmt, of, neg, dev, _bad(items, par, ep))
    assert not out[res == 0].any() and not par[res == 0].any()


def _conv_items(edge, rnd, fmt, n):
    """n items of one input format: the whole edge list of that format first, then seeded valid and corrupted ones"""
    items = [x for x in edge["convert"] if x[1] == fmt]
    fill = [x for x in rnd["convert"] if x[1] == fmt]
    items = items + _cycle(fill, n - len(items)) if n > len(items) else items[:n]
    return items


def test_convert_every_format_pair(engine, edge, rnd):
    """all 5 x 6 format pairs on 257 items that mix valid and refused keys (every refusal edge of the input format among them), plain and
    negated, host and _dev forms; parities_out everywhere"""
    for fmt in range(5):
        items = _conv_items(edge, rnd, fmt, 257)
        assert len(items) == 257 and 0 < sum(x[3] for x in items) < 257
        for of in range(6):
            _conv_check(engine, items, fmt, of, 0)
            _conv_check(engine, items, fmt, of, 1)
            _conv_check(engine, items, fmt, of, (fmt + of) & 1, dev=True)


def test_convert_refusal_edges_are_in_the_list(edge):
    names = {x[0]: x[3] for x in edge["convert"]}
    want0 = ["fmt 0 x = p", "fmt 0 x = 0", "fmt 0 x = 2^256 - 1", "fmt 2 prefix 02 x = p", "fmt 2 prefix 03 x = 0", "fmt 2 bad prefix 00", "fmt 2 bad prefix 01",
             "fmt 2 bad prefix 04", "fmt 2 bad prefix 05", "fmt 3 bad prefix 02", "fmt 3 bad prefix 05", "fmt 3 prefix 06 with odd y", "fmt 3 prefix 07 with even y",
             "fmt 3 y = p", "fmt 4 y = p", "fmt 3 y off the curve", "fmt 4 y off the curve", "fmt 4 y = 2^256 - 1", "all-zero object", "fmt 4 x = p", "fmt 3 x = p"]
    for nm in want0:
        assert names[nm] == 0, nm
    assert any(k.endswith("not on the curve") and v == 0 for k, v in names.items())
    for nm in ("fmt 3 y replaced by p - y", "fmt 4 y replaced by p - y", "object with odd y (to format 5: y is made even)", "valid odd y hybrid", "valid even y hybrid"):
        assert names[nm] == 1, nm
    assert "fmt 0 x = p - 1" in names and "fmt 2 prefix 02 x = p - 1" in names            # (whether p - 1 is on the curve is the reference's to say)


def test_convert_sizes_and_sub_ranges(engine, eng512, edge, rnd):
    """1, 64 and 65 items (a full wavefront, one lane beyond it), and 1 100 items as three launches of 512 lanes"""
    for fmt, of in ((2, 1), (1, 2), (4, 5), (0, 3), (3, 0)):
        for n in (1, 64, 65):
            items = _conv_items(edge, rnd, fmt, 400)[-n:]
            _conv_check(engine, items, fmt, of, 0)
            _conv_check(engine, items, fmt, of, 1, dev=True)
        items = _conv_items(edge, rnd, fmt, 1100)
        _conv_check(eng512, items, fmt, of, 0)
        _conv_check(eng512, items, fmt, of, 1, dev=True)
    # no parities wanted: NULL
    items = _conv_items(edge, rnd, 2, 65); keys = _arr([x[2] for x in items], 33)
    d_res, d_out, _ = _fill(65, 64)
    engine.pubkey_convert_dev(d_res, d_out, _dev(keys), 2, 1)
    engine.sync()
    er, eo, _ = _conv_expect(items, 1, 0)
    assert np.array_equal(d_res.cpu().numpy(), er) and np.array_equal(d_out.cpu().numpy(), eo)


# ---- tweak_mul -------------------------------------------------------------------------------------------------------------------------------
def _tm_check(call, items, fmt, of):
    keys = _arr([x[2] for x in items], PK_BYTES[fmt]); t = _arr([x[3] for x in items], 32)
    res, out, par = call(keys, t, fmt, of)
    er = np.array([x[4] for x in items], np.int32); eo = _arr([x[5][of] for x in items], PK_BYTES[of]); ep = np.array([x[6] for x in items], np.uint8)
    assert np.array_equal(res, er), (fmt, of, _bad(items, res, er))
    assert np.array_equal(out, eo), (fmt, of, _bad(items, out, eo))
    assert np.array_equal(par, ep), (fmt, of, _bad(items, par, ep))


def _tm_host(engine):
    return lambda keys, t, fmt, of: engine.pubkey_tweak_mul(keys, t, key_format=fmt, out_format=of)


def _tm_dev(engine):
    def call(keys, t, fmt, of):
        d_res, d_out, d_par = _fill(t.shape[0], PK_BYTES[of])
        engine.pubkey_tweak_mul_dev(d_res, d_out, _dev(keys), _dev(t), key_format=fmt, out_format=of, parities_out=d_par)
        engine.sync()
        return d_res.cpu().numpy(), d_out.cpu().numpy(), d_par.cpu().numpy()
    return call


def test_tweak_mul_edges(engine, edge):
    """tweaks 0, 1, 2, n - 1, n, n + 1, 2^256 - 1, lambda (one half of the split is zero), 2^128 and refused keys, on keys in formats 0 .. 4"""
    from tests.pubkey_ref import TWEAKS
    assert {nm for nm, _ in TWEAKS} >= {"0", "1", "2", "n-1", "n", "n+1", "2^256-1", "lambda", "2^128"}
    for fmt in range(5):
        items = [x for x in edge["tweak_mul"] if x[1] == fmt]
        assert len(items) >= len(TWEAKS) and 0 < sum(x[4] for x in items) < len(items)
        _tm_check(_tm_host(engine), items, fmt, 1)
        _tm_check(_tm_host(engine), items, fmt, (fmt + 2) % 6)
        _tm_check(_tm_dev(engine), items, fmt, 4 if fmt != 4 else 5)


def test_tweak_mul_shapes(engine, eng512, edge, rnd):
    """n = 1; 65 items of which only lane 64, and only lane 0, has a product (the inversion and ecmult_lane are wave-wide); 1 100 items as
    three launches of 512 lanes"""
    valid = [x for x in edge["tweak_mul"] + rnd["tweak_mul"] if x[1] == 1 and x[4] == 1]
    dead = [x for x in edge["tweak_mul"] if x[1] == 1 and x[4] == 0]
    assert len(valid) >= 50 and len(dead) >= 4
    for call in (_tm_host(engine), _tm_dev(engine)):
        _tm_check(call, valid[:1], 1, 1)
        _tm_check(call, dead[:1], 1, 1)
        _tm_check(call, _cycle(dead, 64) + valid[:1], 1, 2)
        _tm_check(call, valid[1:2] + _cycle(dead, 64), 1, 2)
    for fmt in (1, 2):
        items = _cycle([x for x in edge["tweak_mul"] + rnd["tweak_mul"] if x[1] == fmt], 1100)
        assert 0 < sum(x[4] for x in items) < 1100
        _tm_check(_tm_host(eng512), items, fmt, 1)
        _tm_check(_tm_dev(eng512), items, fmt, 0)


def test_tweak_mul_group(edge, rnd):
    """the group form on two engines (of device 0 where the node has one GPU): the shares 150 / 150, 1 / 2 and a lone item"""
    import torch
    from secp256k1_zkp_amd import Group
    g = Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0])
    try:
        call = lambda keys, t, fmt, of: g.pubkey_tweak_mul(keys, t, key_format=fmt, out_format=of)      # noqa: E731
        for fmt in (1, 2, 4):
            items = _cycle([x for x in edge["tweak_mul"] + rnd["tweak_mul"] if x[1] == fmt], 300)
            _tm_check(call, items, fmt, 1)
            _tm_check(call, items[:3], fmt, 2)
            _tm_check(call, items[:1], fmt, 5)
    finally:
        g.close()


# ---- combine ---------------------------------------------------------------------------------------------------------------------------------
def _comb_arrays(items):
    fmt = items[0][1]
    assert all(x[1] == fmt for x in items)
    keys = np.frombuffer(b"".join(b"".join(x[2]) for x in items), np.uint8).copy()
    off = np.zeros(len(items) + 1, np.uint64); off[1:] = np.cumsum([len(x[2]) for x in items])
    return fmt, keys, off


def _comb_check(engine, items, of, dev=False):
    fmt, keys, off = _comb_arrays(items); n = len(items)
    if dev:
        d_res, d_out, d_par = _fill(n, PK_BYTES[of])
        engine.pubkey_combine_dev(d_res, d_out, _dev(keys) if keys.size else None, off, key_format=fmt, out_format=of, parities_out=d_par)
        engine.sync()
        res, out, par = d_res.cpu().numpy(), d_out.cpu().numpy(), d_par.cpu().numpy()
    else:
        res, out, par = engine.pubkey_combine(keys, off, key_format=fmt, out_format=of)
    er = np.array([x[3] for x in items], np.int32); eo = _arr([x[4][of] for x in items], PK_BYTES[of]); ep = np.array([x[5] for x in items], np.uint8)
    assert np.array_equal(res, er), (fmt, of, dev, _bad(items, res, er))
    assert np.array_equal(out, eo), (fmt, of, dev, _bad(items, out, eo))
    assert np.array_equal(par, ep), (fmt, of, dev, _bad(items, par, ep))


def test_combine_edges(engine, edge):
    """set sizes 0, 1, 2, 3, F - 1, F, F + 1, 2F + 1 and F * F + 1 (three levels); [P, P], [P, Q, P+Q] (a doubling against a Jacobian
    accumulator), [P, -P], [P, -P, Q] (infinity in mid-chain), [P, Q, -(P+Q)]; 2F keys whose second chunk repeats / negates the first (a
    doubling / infinity in the second pass); a refused key first, last and at a chunk boundary; every input format"""
    sizes = {len(x[2]) for x in edge["combine"] if x[1] == 1}
    assert sizes >= {0, 1, 2, 3, F - 1, F, F + 1, 2 * F + 1, F * F + 1}
    for fmt in range(5):
        items = [x for x in edge["combine"] if x[1] == fmt]
        assert 0 < sum(x[3] for x in items) < len(items)
        _comb_check(engine, items, 1)
        _comb_check(engine, items, 2, dev=True)
        for x in items[:3] + items[-2:]:                       # and alone: n_sets = 1
            _comb_check(engine, [x], 4)


def test_combine_chunk_length_two(edge):
    """the test switch: S2K_OPT_PUBKEY_FOLD_FANIN = 2, sizes 1 .. 9 (up to four levels) and the rest of the edge list; then 3 and 64"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        items = [x for x in edge["combine"] if x[1] == 1]
        assert {len(x[2]) for x in items} >= set(range(1, 10))
        for fanin in (2, 3, 64):
            eng.set_option(Engine.OPT_PUBKEY_FOLD_FANIN, fanin)
            _comb_check(eng, items, 1)
            _comb_check(eng, items, 0, dev=True)
        for v in (1, 65):
            assert eng._lib.s2k_engine_set_option(eng._h, Engine.OPT_PUBKEY_FOLD_FANIN, v) == 0 and eng._lib.s2k_last_status() == 2
        eng.set_option(Engine.OPT_MUSIG_SUM_FANIN, 2)          # the MuSig switch does not touch this call
        eng.set_option(Engine.OPT_PUBKEY_FOLD_FANIN, 16)
        _comb_check(eng, items, 1)
    finally:
        eng.close()


def _ragged(pref, rnd, fmt, sizes, seed):
    from tests.pubkey_ref import combine_item
    rng = np.random.default_rng(seed)
    pool = [x[2] for x in rnd["convert"] if x[1] == fmt and x[3] == 1]
    assert len(pool) >= 20
    return [combine_item(pref, f"ragged {k}", fmt, [pool[int(rng.integers(0, len(pool)))] for _ in range(m)]) for k, m in enumerate(sizes)]


def test_combine_ragged_batches(engine, eng512, pref, rnd):
    """n_sets 1, 65 and 300 with empty sets in first, middle and last position, in every input format; on the 512-lane engine the 300
    sets hold more chunks than one launch takes, at the default chunk length and at 2"""
    from secp256k1_zkp_amd import Engine
    rng = np.random.default_rng(7707)
    for fmt in range(5):
        sizes = [int(v) for v in rng.integers(0, 6, 65)]; sizes[0] = 0; sizes[31] = 0; sizes[64] = 0; sizes[1] = F + 3
        items = _ragged(pref, rnd, fmt, sizes, 7708 + fmt)
        _comb_check(engine, items, 1)
        _comb_check(engine, items, 3, dev=True)
        _comb_check(engine, items[1:2], 1)
    sizes = [int(v) for v in rng.integers(0, 60, 300)]; sizes[0] = 0; sizes[150] = 0; sizes[299] = 0; sizes[7] = 2 * F * F + 5
    items = _ragged(pref, rnd, 1, sizes, 7720)
    assert sum(-(-m // F) for m in sizes) > 512 and sum(sizes) > 4096
    _comb_check(engine, items, 1)
    _comb_check(eng512, items, 1)
    _comb_check(eng512, items, 2, dev=True)
    try:
        eng512.set_option(Engine.OPT_PUBKEY_FOLD_FANIN, 2)     # 512-lane launches in every pass
        _comb_check(eng512, items, 1)
    finally:
        eng512.set_option(Engine.OPT_PUBKEY_FOLD_FANIN, F)


# ---- the C ABI's argument checks -----------------------------------------------------------------------------------------------------------------
def test_batch_argument_checks(engine, edge):
    """NULL arrays, unknown formats and bad offsets fail the call with the argument status and leave zeroed outputs; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    items = [x for x in edge["convert"] if x[1] == 1 and x[3] == 1][:4]
    keys = _arr([x[2] for x in items], 64); t = np.tile(np.arange(1, 33, dtype=np.uint8), (4, 1))
    res = np.full(4, 7, np.int32); out = np.full((4, 65), 0xFF, np.uint8); par = np.full(4, 0xFF, np.uint8)
    for fn in (L.secp256k1_ec_pubkey_convert_batch, L.secp256k1_ec_pubkey_negate_batch):
        good = [p(res), p(out), 1, p(par), p(keys), 1, 4]
        assert fn(h, *good) == 1 and res.all()
        for k in (0, 1, 4):
            a = list(good); a[k] = None
            assert fn(h, *a) == 0 and L.s2k_last_status() == 2, k
        a = list(good); a[3] = None
        assert fn(h, *a) == 1                                  # parities_out is optional
        for of, f in ((6, 1), (-1, 1), (1, 5), (1, -1)):
            res[:] = 7; par[:] = 0xFF
            a = list(good); a[2] = of; a[5] = f
            assert fn(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any() and not par.any(), (of, f)
        a = list(good); a[6] = 0
        assert fn(h, *a) == 1 and fn(h, None, None, 9, None, None, 9, 0) == 1
    good = [p(res), p(out), 1, p(par), p(keys), 1, p(t), 4]
    assert L.secp256k1_ec_pubkey_tweak_mul_batch(h, *good) == 1 and res.all()
    for k in (0, 1, 4, 6):
        a = list(good); a[k] = None
        assert L.secp256k1_ec_pubkey_tweak_mul_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
    for of, f in ((6, 1), (1, 5)):
        a = list(good); a[2] = of; a[5] = f
        assert L.secp256k1_ec_pubkey_tweak_mul_batch(h, *a) == 0 and L.s2k_last_status() == 2
        assert L.secp256k1_ec_pubkey_tweak_mul_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ec_pubkey_tweak_mul_batch(h, None, None, 1, None, None, 1, None, 0) == 1
    off = np.array([0, 1, 4], np.uint64)
    good = [p(res), p(out), 1, p(par), p(keys), 1, p(off), 2]
    assert L.secp256k1_ec_pubkey_combine_batch(h, *good) == 1 and res[:2].all()
    for k in (0, 1, 4, 6):
        a = list(good); a[k] = None
        assert L.secp256k1_ec_pubkey_combine_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
    for bad in ([1, 2, 4], [0, 3, 2]):                         # not starting at 0, decreasing
        res[:] = 7
        b = np.array(bad, np.uint64); a = list(good); a[6] = p(b)
        assert L.secp256k1_ec_pubkey_combine_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res[:2].any(), bad
        assert L.secp256k1_ec_pubkey_combine_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, bad
    for of, f in ((6, 1), (1, 5)):
        a = list(good); a[2] = of; a[5] = f
        assert L.secp256k1_ec_pubkey_combine_batch(h, *a) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ec_pubkey_combine_batch(h, None, None, 1, None, None, 1, None, 0) == 1
    zero = np.zeros(3, np.uint64)                              # two empty sets and no key array at all
    assert L.secp256k1_ec_pubkey_combine_batch(h, p(res), p(out), 1, p(par), None, 1, p(zero), 2) == 1 and not res[:2].any()
    assert L.secp256k1_ec_pubkey_tweak_mul_batch_group(None, *good) == 0


# ---- chaining and the single-item forms ----------------------------------------------------------------------------------------------------------
def test_recover_convert_ecmult_convert_stays_on_the_device(engine, pref, ref):
    """secp256k1_ecdsa_recover_batch_dev -> convert (object -> x | y) -> s2k_ecmult_batch_dev -> convert (x | y -> compressed) on 65 items,
    with no host copy in between; the reference recovers, multiplies (secp256k1_ec_pubkey_tweak_mul) and serialises the same items"""
    import torch
    from tests.ecdsa_ref import EcdsaRef
    eref = EcdsaRef()
    rng = np.random.default_rng(7709)
    n = 65
    msgs, sigs, recids, _ = eref.make_recoverable(n, rng)
    sigs[5, 3] ^= 1; sigs[64, 40] ^= 0x10                       # (recover to other keys, or to none)
    na = rng.integers(0, 256, (n, 32), dtype=np.uint8); na[:, 0] &= 0x7F
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_obj = torch.full((n, 64), 0xFF, dtype=torch.uint8, device="cuda:0")
    engine.ecdsa_recover_batch_dev(d_res, d_obj, _dev(sigs), _dev(recids), _dev(msgs))
    d_res2, d_xy, _ = _fill(n, 64)
    engine.pubkey_convert_dev(d_res2, d_xy, d_obj, 1, 4)
    d_rxy = torch.zeros((n, 64), dtype=torch.uint8, device="cuda:0"); d_inf = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    engine.sync()                                               # (torch works on its own stream: order it behind the engine's, and back)
    d_ainf = (d_res2 == 0).to(torch.uint8)                      # a key that was not recovered enters the multiplication as infinity
    torch.cuda.synchronize()
    engine.ecmult_batch_dev(d_rxy, d_inf, d_xy, _dev(na), a_inf=d_ainf)
    d_res3, d_ser, d_par = _fill(n, 33)
    engine.pubkey_convert_dev(d_res3, d_ser, d_rxy, 4, 2, parities_out=d_par)
    engine.sync()
    rexp, robj = eref.recover_many(sigs, recids, msgs)
    assert np.array_equal(d_res.cpu().numpy(), rexp) and np.array_equal(d_res2.cpu().numpy(), rexp) and rexp.sum() >= 60
    got, ser, par = d_res3.cpu().numpy(), d_ser.cpu().numpy(), d_par.cpu().numpy()
    for i in range(n):
        prod = pref.ec_tweak_mul(robj[i].tobytes(), na[i].tobytes()) if rexp[i] else None
        outs, p = pref.outs(prod)
        assert got[i] == int(prod is not None) and ser[i].tobytes() == outs[2] and par[i] == p, i


def test_single_item_forms_have_the_reference_argument_lists(engine, edge, pref):
    """the eight _amd forms on the edge lists, called as the reference's functions are: opaque objects in, the reference's verdict and bytes out"""
    L = engine._lib
    S = L.s2k_last_status
    for name, fmt, key, v, outs, par, nouts, npar in edge["convert"]:
        if fmt in (2, 3):
            o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
            assert L.secp256k1_ec_pubkey_parse_amd(None, o, key, len(key)) == v and o.raw == outs[1] and S() == 0, name
        if fmt == 0:
            o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
            assert L.secp256k1_xonly_pubkey_parse_amd(None, o, key) == v and o.raw == outs[1] and S() == 0, name
        if fmt == 1:
            for flags, of in ((258, 2), (2, 3)):
                o = ctypes.create_string_buffer(b"\xAA" * 70, 70); ln = ctypes.c_size_t(70)
                assert L.secp256k1_ec_pubkey_serialize_amd(None, o, ctypes.byref(ln), key, flags) == v and S() == 0, name
                assert ln.value == (PK_BYTES[of] if v else 0) and o.raw == (outs[of] + bytes(70 - PK_BYTES[of]) if v else bytes(70)), name
            io = ctypes.create_string_buffer(key, 64)
            assert L.secp256k1_ec_pubkey_negate_amd(None, io) == v and io.raw == nouts[1] and S() == 0, name
            o = ctypes.create_string_buffer(b"\xAA" * 32, 32)
            assert L.secp256k1_xonly_pubkey_serialize_amd(None, o, key) == v and o.raw == outs[0] and S() == 0, name
            o = ctypes.create_string_buffer(b"\xAA" * 64, 64); pp = ctypes.c_int(9)
            assert L.secp256k1_xonly_pubkey_from_pubkey_amd(None, o, ctypes.byref(pp), key) == v and S() == 0, name
            assert (o.raw == outs[5] and pp.value == par) if v else (o.raw == b"\xAA" * 64 and pp.value == 9), name
            if v:
                assert L.secp256k1_xonly_pubkey_from_pubkey_amd(None, o, None, key) == 1 and o.raw == outs[5]
    assert sum(1 for x in edge["convert"] if x[1] == 1) >= 4
    for name, fmt, key, t, v, outs, par in [x for x in edge["tweak_mul"] if x[1] == 1]:
        io = ctypes.create_string_buffer(key, 64)
        assert L.secp256k1_ec_pubkey_tweak_mul_amd(None, io, t) == v and io.raw == outs[1] and S() == 0, name
    for name, fmt, keys, v, outs, par in [x for x in edge["combine"] if x[1] == 1 and 1 <= len(x[2]) <= 2 * F + 1]:
        bufs = [ctypes.create_string_buffer(k, 64) for k in keys]
        ptrs = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
        o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_ec_pubkey_combine_amd(None, o, ptrs, len(bufs)) == v and o.raw == outs[1] and S() == 0, name
    # the output may be one of the inputs (the reference reads every key before it writes)
    Pk, Q = [x for x in edge["combine"] if x[0] == "2 keys"][0][2]
    a = ctypes.create_string_buffer(Pk, 64); b = ctypes.create_string_buffer(Q, 64)
    ptrs = (ctypes.c_void_p * 2)(ctypes.addressof(a), ctypes.addressof(b))
    assert L.secp256k1_ec_pubkey_combine_amd(None, a, ptrs, 2) == 1 and a.raw == pref.ec_combine([Pk, Q])
