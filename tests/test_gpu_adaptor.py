"""GPU: ECDSA adaptor-signature verification and the two-point multiplication (csrc/adaptor.h, csrc/ecmult.h: ecmult_lane2,
csrc/engine_adaptor.hip).  The verdicts are the reference's own where they are recorded (tests/golden/adaptor_vectors.json) and the Python
model's (tests/adaptor_ref.py, which agrees with the reference on every recorded item) elsewhere; the two-point multiplication is
compared with the reference's secp256k1_ecmult_multi_var (oracle/_ref) item by item."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import adaptor_ref as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEY_BYTES = {0: 33, 1: 64, 2: 65}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def golden():
    return A.from_json(json.load(open(os.path.join(HERE, "golden", "adaptor_vectors.json")))["vectors"])


@pytest.fixture(scope="module")
def edge():
    return A.edge_cases()


@pytest.fixture(scope="module")
def pool():
    """200 seeded items, one in eight corrupted; the batches below are cut from it (cyclically for the largest) and never change it"""
    items = A.random_items(200, 5510, corrupt_every=8)
    ones = sum(x[5] for x in items)
    assert ones == 175                                                                    # every uncorrupted item is valid, every flipped bit fatal
    return items


def _take(pool, n, start=0):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def _arrays(items, fmt):
    """items that exist in pk_format fmt -> (kept items, sigs, pubkeys, msgs, enckeys, expected verdicts)"""
    kept, pks, eks = [], [], []
    for it in items:
        keys = A.keys_in_format(it, fmt)
        if keys is not None:
            kept.append(it); pks.append(keys[0]); eks.append(keys[1])
    n = len(kept)
    arr = lambda bs, w: np.frombuffer(b"".join(bs), np.uint8).reshape(n, w).copy()      # noqa: E731
    return (kept, arr([x[1] for x in kept], 162), arr(pks, KEY_BYTES[fmt]), arr([x[3] for x in kept], 32), arr(eks, KEY_BYTES[fmt]),
            np.array([x[5] for x in kept], np.int32))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _names(items, got, exp):
    return [x[0] for x, g, e in zip(items, got, exp) if g != e]


def _verify_dev(engine, sigs, pks, msgs, eks, fmt, stream=None):
    import torch
    d_res = torch.full((sigs.shape[0],), 7, dtype=torch.int32, device="cuda:0")
    engine.ecdsa_adaptor_verify_batch_dev(d_res, _dev(sigs), _dev(pks), _dev(msgs), _dev(eks), pk_format=fmt, stream=stream)
    return d_res


def test_golden_fixture_one_batch(engine, golden):
    """every recorded item in one batch per key format: the reference's verdicts"""
    for fmt in (0, 1, 2):
        items, sigs, pks, msgs, eks, exp = _arrays(golden, fmt)
        assert len(items) >= 90 and 0 < exp.sum() < len(items)
        got = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
        assert np.array_equal(got, exp), (fmt, _names(items, got, exp))


def test_edge_list_all_formats_host_dev_group_amd(engine, edge):
    """the edge list in the three key formats through the host and _dev forms (the latter on a caller's stream, into results pre-filled
    with 7), through a group of one engine, and item by item through the _amd form (64-byte objects)"""
    import torch
    from secp256k1_zkp_amd import Group
    g = Group([0])
    s = torch.cuda.Stream()
    try:
        for fmt in (0, 1, 2):
            items, sigs, pks, msgs, eks, exp = _arrays(edge, fmt)
            assert exp.sum() == len(A.EDGE_VERDICTS) and len(items) >= 27
            got = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
            assert np.array_equal(got, exp), (fmt, _names(items, got, exp))
            s.wait_stream(torch.cuda.current_stream())
            d_res = _verify_dev(engine, sigs, pks, msgs, eks, fmt, stream=ctypes.c_void_p(s.cuda_stream))
            s.synchronize()
            got = d_res.cpu().numpy()
            assert np.array_equal(got, exp), (fmt, _names(items, got, exp))
            got = g.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
            assert np.array_equal(got, exp), (fmt, _names(items, got, exp))
        L = engine._lib
        items, sigs, pks, msgs, eks, exp = _arrays(edge, 1)
        assert any(x[6] == 1 for x in items)                                              # the all-zero objects are among them
        for i, it in enumerate(items):
            assert L.secp256k1_ecdsa_adaptor_verify_amd(None, it[1], pks[i].tobytes(), it[3], eks[i].tobytes()) == it[5] and L.s2k_last_status() == 0, it[0]
    finally:
        g.close()


def test_batch_argument_checks(engine, edge):
    """NULL where the reference has ARG_CHECK and a pk_format out of range fail the call with the argument status; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    items, sigs, pks, msgs, eks, exp = _arrays(edge[:4], 0)
    res = np.full(4, 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(sigs), p(pks), p(msgs), p(eks), 0, 4]
    assert L.secp256k1_ecdsa_adaptor_verify_batch(h, *good) == 1 and np.array_equal(res, exp)
    for k in (0, 1, 2, 3, 4):
        a = list(good); a[k] = None
        assert L.secp256k1_ecdsa_adaptor_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
        assert L.secp256k1_ecdsa_adaptor_verify_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, k
    for fmt in (3, -1):
        a = list(good); a[5] = fmt
        assert L.secp256k1_ecdsa_adaptor_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any(), fmt
        assert L.secp256k1_ecdsa_adaptor_verify_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, fmt
    assert L.secp256k1_ecdsa_adaptor_verify_batch(h, None, None, None, None, None, 0, 0) == 1
    assert L.secp256k1_ecdsa_adaptor_verify_batch_dev(h, None, None, None, None, None, None, 0, 0) == 1
    assert L.s2k_ecmult2_batch(h, None, None, None, None, None, None, None, None, 0) == 1
    assert L.s2k_ecmult2_batch(h, None, None, None, None, None, None, None, None, 1) == 0 and L.s2k_last_status() == 2
    assert engine.ecdsa_adaptor_verify_batch(b"", b"", b"", b"").size == 0


def test_batch_sizes(engine, pool):
    """1 .. 1000 items, one in eight corrupted: wavefront and block edges, the dead lanes of a partial last wavefront"""
    for n in SIZES:
        items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, n, start=n), 0)
        assert len(items) == n and (n < 8 or 0 < exp.sum() < n)
        got = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=0)
        assert np.array_equal(got, exp), (n, np.flatnonzero(got != exp)[:8])
    for fmt in (1, 2):                                                                    # (an item whose flipped bit broke a key has no object form)
        items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, 257), fmt)
        assert len(items) >= 240 and 0 < exp.sum() < len(items)
        got = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
        assert np.array_equal(got, exp), (fmt, _names(items, got, exp))


def test_sub_range_launches(engine, pool):
    """700 items on an engine whose launches take 256 and then 512 lanes: sub-range launches, equal to the single-launch results"""
    from secp256k1_zkp_amd import Engine
    items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, 700, start=3), 0)
    one = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=0)
    assert np.array_equal(one, exp) and 0 < exp.sum() < 700
    eng = Engine(0)
    try:
        for lanes in (256, 512):
            eng.set_option(Engine.OPT_MAX_LANES, lanes)
            assert np.array_equal(eng.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=0), one), lanes
            d_res = _verify_dev(eng, sigs, pks, msgs, eks, 0)
            eng.sync()
            assert np.array_equal(d_res.cpu().numpy(), one), lanes
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_one_odd_lane_in_a_valid_wavefront(engine, pool, edge):
    """an item that drives its wavefront out of the lock-step joint form, and a refused key, at lanes 0, 31 and 63 of an otherwise valid
    wavefront (and with a second, untouched wavefront behind it): the odd item reads 0, every neighbour keeps its verdict 1.  Covers the
    divergence out of ecmult_lane2 (a zero scalar makes the wavefront non-uniform; R2 at infinity is an addition that meets the
    accumulator's own x) and the shared inversion (the odd lane hands in 1)."""
    valid = [x for x in pool if x[5] == 1][:128]
    by_name = {x[0]: x for x in edge}
    odd = [by_name["s = 0"], by_name["e = 0"], by_name["R = k2 Y, s = e k2: R2 at infinity"], by_name["R = k2 Y, s = -e k2: the doubling inside R2"],
           by_name["s = e k: R1 at infinity"], by_name["all-zero enckey object"], by_name["all-zero pubkey object"], by_name["prefix 04 on R"]]
    assert all(x[5] == 0 for x in odd)
    for it in odd:
        fmt = 1 if it[6] == 1 else 0
        for lane in (0, 31, 63):
            for n in (64, 128):
                items = list(valid[:n]); items[lane] = it
                kept, sigs, pks, msgs, eks, exp = _arrays(items, fmt)
                assert len(kept) == n and exp.sum() == n - 1 and exp[lane] == 0
                got = engine.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
                assert np.array_equal(got, exp), (it[0], lane, n, np.flatnonzero(got != exp)[:8])


def _ecmult2_reference(ref, a_xy, na, b_xy, nb, a_inf, b_inf):
    n = a_xy.shape[0]
    r = np.zeros((n, 64), np.uint8); inf = np.zeros(n, np.int32)
    for i in range(n):
        rr, ri = ref.ecmult_multi(np.concatenate([na[i], nb[i]]), np.concatenate([a_xy[i], b_xy[i]]),
                                  pt_inf=None if a_inf is None else np.array([a_inf[i], b_inf[i]], np.uint8))
        inf[i] = ri
        if not ri:
            r[i] = rr
    return r, inf


@pytest.fixture(scope="module")
def points(ref):
    """1000 random points and scalars (shared by the sizes below, never changed), with the special cases of the joint form at fixed places"""
    rng = np.random.default_rng(5511)
    n = 1000
    a_xy = np.stack([np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(n)]).copy()
    b_xy = np.stack([np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(n)]).copy()
    na = rng.integers(0, 256, (n, 32), dtype=np.uint8); nb = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a_inf = np.zeros(n, np.uint8); b_inf = np.zeros(n, np.uint8)
    neg = lambda p: np.frombuffer(p[:32].tobytes() + ((A.P - int.from_bytes(p[32:].tobytes(), "big")) % A.P).to_bytes(32, "big"), np.uint8)      # noqa: E731
    sc = lambda v: np.frombuffer(A.b32(v), np.uint8)                                      # noqa: E731
    # wavefront 2 (items 128..191): zero scalars, 1, n-1, A = +-B with equal and opposite scalars, points at infinity
    na[130] = sc(0); nb[131] = sc(0); na[132] = sc(0); nb[132] = sc(0); na[133] = sc(1); nb[133] = sc(A.N - 1); na[134] = sc(A.N - 1); nb[134] = sc(1)
    b_xy[135] = a_xy[135]; nb[135] = na[135]                                              # 2 na A
    b_xy[136] = neg(a_xy[136]); nb[136] = na[136]                                         # infinity
    b_xy[137] = a_xy[137]                                                                 # (na + nb) A
    b_xy[138] = neg(a_xy[138])
    a_inf[139] = 1; b_inf[140] = 1; a_inf[141] = 1; b_inf[141] = 1
    # items 700.., inside otherwise ordinary wavefronts: A = -B with equal scalars (the joint form meets its own x at the last addition)
    for i in (704, 735, 767):
        b_xy[i] = neg(a_xy[i]); nb[i] = na[i]
    exp, exp_inf = _ecmult2_reference(ref, a_xy, na, b_xy, nb, a_inf, b_inf)
    assert exp_inf[[132, 136, 141, 704, 735, 767]].all() and exp_inf.sum() == 6
    return a_xy, na, b_xy, nb, a_inf, b_inf, exp, exp_inf


def test_ecmult2_batch_against_reference(engine, points):
    """s2k_ecmult2_batch at the same sizes: random points and scalars (all finite, NULL flags: the joint form), then ranges that hold the
    special cases with the infinity flags given (zero scalars, A = +-B, points at infinity: the two-call form for their wavefronts)"""
    import torch
    a_xy, na, b_xy, nb, a_inf, b_inf, exp, exp_inf = points
    for n in SIZES:
        lo = 0 if n <= 128 else 1000 - n                                                  # n <= 128: no special item inside; flags not needed
        sl = slice(lo, lo + n)
        flags = {} if n <= 128 else {"a_inf": a_inf[sl], "b_inf": b_inf[sl]}
        r, inf = engine.ecmult2_batch(a_xy[sl], na[sl], b_xy[sl], nb[sl], **flags)
        assert np.array_equal(inf, exp_inf[sl]), (n, np.flatnonzero(inf != exp_inf[sl])[:8])
        assert np.array_equal(r, exp[sl]), (n, np.flatnonzero((r != exp[sl]).any(axis=1))[:8])
    # the _dev form, outputs pre-filled
    sl = slice(100, 400)
    d_r = torch.full((300, 64), 0xFF, dtype=torch.uint8, device="cuda:0"); d_inf = torch.full((300,), 7, dtype=torch.int32, device="cuda:0")
    engine.ecmult2_batch_dev(d_r, d_inf, _dev(a_xy[sl]), _dev(na[sl]), _dev(b_xy[sl]), _dev(nb[sl]), a_inf=_dev(a_inf[sl]), b_inf=_dev(b_inf[sl]))
    engine.sync()
    assert np.array_equal(d_inf.cpu().numpy(), exp_inf[sl]) and np.array_equal(d_r.cpu().numpy(), exp[sl])
