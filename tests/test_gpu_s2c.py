"""GPU: ECDSA sign-to-contract checks, anti-exfil host verification and host commitments (csrc/s2c.h, csrc/engine_s2c.hip).  The verdicts
are the reference's own where they are recorded (tests/golden/s2c_vectors.json) and the Python model's (tests/s2c_ref.py, which agrees with
the reference on every recorded item) elsewhere; the host commitments are hashlib's.  Every comparison is exact."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import s2c_ref as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PK_BYTES = {0: 33, 1: 64, 2: 65}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def golden():
    return S.from_json(json.load(open(os.path.join(HERE, "golden", "s2c_vectors.json")))["vectors"])


@pytest.fixture(scope="module")
def edge():
    return S.edge_cases()


@pytest.fixture(scope="module")
def pool():
    """200 seeded items, one in eight corrupted; the batches below are cut from it (cyclically for the largest) and never change it"""
    items = S.random_items(200, 5610, corrupt_every=8)
    assert sum(x[7] for x in items) == 175                                                # every uncorrupted item is valid, every flipped bit fatal to host_verify
    assert 175 < sum(x[6] for x in items) < 200                                           # but not to the commitment check: s, message and key are not its inputs
    return items


def _take(pool, n, start=0):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def _arrays(items, sf=0, pf=0, of=0):
    """items that exist in this format combination -> dict: kept items, sigs (array, or list of byte strings for DER), msgs, pks, data,
    openings, expected commit and host verdicts"""
    kept, sigs, pks, ops = [], [], [], []
    for it in items:
        got = S.keys_in_format(it, sf, pf, of)
        if got is not None:
            kept.append(it); sigs.append(got[0]); pks.append(got[1]); ops.append(got[2])
    n = len(kept)
    arr = lambda bs, w: np.frombuffer(b"".join(bs), np.uint8).reshape(n, w).copy()      # noqa: E731
    return dict(items=kept, sigs=sigs if sf == 2 else arr(sigs, 64), msgs=arr([x[2] for x in kept], 32), pks=arr(pks, PK_BYTES[pf]), data=arr([x[4] for x in kept], 32),
                ops=arr(ops, 64 if of else 33), commit=np.array([x[6] for x in kept], np.int32), host=np.array([x[7] for x in kept], np.int32), fmt=(sf, pf, of), n=n)


def _commit(obj, a):
    return obj.ecdsa_s2c_verify_commit_batch(a["sigs"], a["data"], a["ops"], sig_format=a["fmt"][0], opening_format=a["fmt"][2])


def _host(obj, a):
    return obj.anti_exfil_host_verify_batch(a["sigs"], a["msgs"], a["pks"], a["data"], a["ops"], sig_format=a["fmt"][0], pk_format=a["fmt"][1], opening_format=a["fmt"][2])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _both_dev(engine, a, stream=None):
    """both verifiers through the _dev forms into results pre-filled with 7"""
    import torch
    from secp256k1_zkp_amd import Engine
    sf, pf, of = a["fmt"]
    sigs, off = a["sigs"], None
    if sf == 2:
        sigs, off = Engine.pack(sigs)
        off = _dev(off.astype(np.int64))
    d_sig, d_msg, d_pk, d_dat, d_op = _dev(sigs), _dev(a["msgs"]), _dev(a["pks"]), _dev(a["data"]), _dev(a["ops"])
    d_c = torch.full((a["n"],), 7, dtype=torch.int32, device="cuda:0"); d_h = torch.full((a["n"],), 7, dtype=torch.int32, device="cuda:0")
    engine.ecdsa_s2c_verify_commit_batch_dev(d_c, d_sig, d_dat, d_op, sig_format=sf, opening_format=of, sig_off=off, n=a["n"], stream=stream)
    engine.anti_exfil_host_verify_batch_dev(d_h, d_sig, d_msg, d_pk, d_dat, d_op, sig_format=sf, pk_format=pf, opening_format=of, sig_off=off, n=a["n"], stream=stream)
    return d_c, d_h


def _names(a, got, exp):
    return [x[0] for x, g, e in zip(a["items"], got, exp) if g != e]


def test_golden_fixture_one_batch_per_format_combination(engine, golden):
    """every recorded item in one batch per combination of signature, key and opening format: the reference's verdicts"""
    for sf, pf, of in S.FORMAT_COMBINATIONS:
        a = _arrays(golden, sf, pf, of)
        assert a["n"] >= 60 and 0 < a["host"].sum() < a["commit"].sum() < a["n"]
        got = _host(engine, a)
        assert np.array_equal(got, a["host"]), (a["fmt"], _names(a, got, a["host"]))
        if pf == 0:
            got = _commit(engine, a)
            assert np.array_equal(got, a["commit"]), (a["fmt"], _names(a, got, a["commit"]))


def test_edge_list_host_dev_group_amd(engine, edge):
    """the edge list through the host and _dev forms (the latter on a caller's stream, into results pre-filled with 7), through a group of
    one engine, and item by item through the _amd forms (64-byte objects)"""
    import torch
    from secp256k1_zkp_amd import Group
    g = Group([0])
    s = torch.cuda.Stream()
    seen = set()
    try:
        for fmt in ((0, 0, 0), (1, 1, 1), (2, 2, 0), (0, 1, 1), (1, 2, 0), (2, 0, 1)):
            a = _arrays(edge, *fmt)
            seen |= {x[0] for x in a["items"]}
            assert a["n"] >= 16 and a["host"].sum() >= 2 and a["commit"].sum() > a["host"].sum()
            for obj in (engine, g):
                got = _commit(obj, a)
                assert np.array_equal(got, a["commit"]), (fmt, _names(a, got, a["commit"]))
                got = _host(obj, a)
                assert np.array_equal(got, a["host"]), (fmt, _names(a, got, a["host"]))
            s.wait_stream(torch.cuda.current_stream())
            d_c, d_h = _both_dev(engine, a, stream=ctypes.c_void_p(s.cuda_stream))
            s.synchronize()
            assert np.array_equal(d_c.cpu().numpy(), a["commit"]), (fmt, _names(a, d_c.cpu().numpy(), a["commit"]))
            assert np.array_equal(d_h.cpu().numpy(), a["host"]), (fmt, _names(a, d_h.cpu().numpy(), a["host"]))
        assert seen == {x[0] for x in edge}                                               # every edge item ran in some combination
        L = engine._lib
        a = _arrays(edge, 1, 1, 1)
        assert {x[8] for x in a["items"]} >= {"obj_sig", "obj_pubkey", "obj_opening"}     # the objects no parser produces are among them
        for i, it in enumerate(a["items"]):
            sig, pk, op = a["sigs"][i].tobytes(), a["pks"][i].tobytes(), a["ops"][i].tobytes()
            assert L.secp256k1_ecdsa_s2c_verify_commit_amd(None, sig, it[4], op) == it[6] and L.s2k_last_status() == 0, it[0]
            assert L.secp256k1_anti_exfil_host_verify_amd(None, sig, it[2], pk, it[4], op) == it[7] and L.s2k_last_status() == 0, it[0]
    finally:
        g.close()


def test_batch_argument_checks(engine, edge):
    """NULL where the reference has ARG_CHECK and a format out of range fail the call with the argument status; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    a = _arrays(edge[:4], 0, 0, 0)
    res = np.full(4, 7, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(a["sigs"]), None, 0, p(a["data"]), p(a["ops"]), 0, 4]
    assert L.secp256k1_ecdsa_s2c_verify_commit_batch(h, *good) == 1 and np.array_equal(res, a["commit"])
    for k in (0, 1, 4, 5):
        b = list(good); b[k] = None
        assert L.secp256k1_ecdsa_s2c_verify_commit_batch(h, *b) == 0 and L.s2k_last_status() == 2, k
        assert L.secp256k1_ecdsa_s2c_verify_commit_batch_dev(h, None, *b) == 0 and L.s2k_last_status() == 2, k
    for k, bad in ((3, 3), (3, -1), (6, 2), (6, -1), (3, 2)):                            # (sig_format 2 without offsets: a NULL array)
        b = list(good); b[k] = bad; res[:] = 7
        assert L.secp256k1_ecdsa_s2c_verify_commit_batch(h, *b) == 0 and L.s2k_last_status() == 2 and (bad == 2 and k == 3 or not res.any()), (k, bad)
        assert L.secp256k1_ecdsa_s2c_verify_commit_batch_dev(h, None, *b) == 0 and L.s2k_last_status() == 2, (k, bad)
    good = [p(res), p(a["sigs"]), None, 0, p(a["msgs"]), p(a["pks"]), 0, p(a["data"]), p(a["ops"]), 0, 4]
    assert L.secp256k1_anti_exfil_host_verify_batch(h, *good) == 1 and np.array_equal(res, a["host"])
    for k in (0, 1, 4, 5, 7, 8):
        b = list(good); b[k] = None
        assert L.secp256k1_anti_exfil_host_verify_batch(h, *b) == 0 and L.s2k_last_status() == 2, k
        assert L.secp256k1_anti_exfil_host_verify_batch_dev(h, None, *b) == 0 and L.s2k_last_status() == 2, k
    for k, bad in ((3, 3), (3, -1), (6, 3), (6, -1), (9, 2), (9, -1)):
        b = list(good); b[k] = bad; res[:] = 7
        assert L.secp256k1_anti_exfil_host_verify_batch(h, *b) == 0 and L.s2k_last_status() == 2 and not res.any(), (k, bad)
        assert L.secp256k1_anti_exfil_host_verify_batch_dev(h, None, *b) == 0 and L.s2k_last_status() == 2, (k, bad)
    out = np.zeros(32, np.uint8)
    assert L.secp256k1_ecdsa_anti_exfil_host_commit_batch(h, None, p(out), 1) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ecdsa_anti_exfil_host_commit_batch(h, p(out), None, 1) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(h, None, None, p(out), 1) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ecdsa_s2c_verify_commit_batch(h, None, None, None, 0, None, None, 0, 0) == 1
    assert L.secp256k1_ecdsa_s2c_verify_commit_batch_dev(h, None, None, None, None, 0, None, None, 0, 0) == 1
    assert L.secp256k1_anti_exfil_host_verify_batch(h, None, None, None, 0, None, None, 0, None, None, 0, 0) == 1
    assert L.secp256k1_anti_exfil_host_verify_batch_dev(h, None, None, None, None, 0, None, None, 0, None, None, 0, 0) == 1
    assert L.secp256k1_ecdsa_anti_exfil_host_commit_batch(h, None, None, 0) == 1
    assert engine.ecdsa_s2c_verify_commit_batch(b"", b"", b"").size == 0 and engine.anti_exfil_host_verify_batch(b"", b"", b"", b"", b"").size == 0


def test_batch_sizes(engine, pool):
    """1 .. 1000 items, one in eight corrupted: wavefront and block edges, the dead lanes of a partial last wavefront"""
    for n in SIZES:
        a = _arrays(_take(pool, n, start=n), 0, 0, 0)
        assert a["n"] == n and (n < 8 or 0 < a["host"].sum() < a["commit"].sum() <= n)
        got = _host(engine, a)
        assert np.array_equal(got, a["host"]), (n, np.flatnonzero(got != a["host"])[:8])
        got = _commit(engine, a)
        assert np.array_equal(got, a["commit"]), (n, np.flatnonzero(got != a["commit"])[:8])
    for fmt in ((1, 1, 1), (2, 2, 0)):                                                    # (an item whose flipped bit broke a parser has no object form)
        a = _arrays(_take(pool, 257), *fmt)
        assert a["n"] >= 240 and 0 < a["host"].sum() < a["n"]
        got = _host(engine, a)
        assert np.array_equal(got, a["host"]), (fmt, _names(a, got, a["host"]))
        got = _commit(engine, a)
        assert np.array_equal(got, a["commit"]), (fmt, _names(a, got, a["commit"]))


def test_sub_range_launches(engine, pool):
    """700 items on an engine whose launches take 256 and then 512 lanes: sub-range launches, equal to the single-launch results; compact
    and DER signatures (the latter: every launch reads its own window of the offsets)"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        for fmt in ((0, 0, 0), (2, 0, 0)):
            a = _arrays(_take(pool, 700, start=3), *fmt)
            one_c, one_h = _commit(engine, a), _host(engine, a)
            assert np.array_equal(one_c, a["commit"]) and np.array_equal(one_h, a["host"]) and 0 < a["host"].sum() < a["commit"].sum() < a["n"]
            for lanes in (256, 512):
                eng.set_option(Engine.OPT_MAX_LANES, lanes)
                assert np.array_equal(_commit(eng, a), one_c) and np.array_equal(_host(eng, a), one_h), (fmt, lanes)
                d_c, d_h = _both_dev(eng, a)
                eng.sync()
                assert np.array_equal(d_c.cpu().numpy(), one_c) and np.array_equal(d_h.cpu().numpy(), one_h), (fmt, lanes)
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_one_odd_lane_in_a_valid_wavefront(engine, pool, edge):
    """a (1, 0) item, a (0, 0) item, a refused opening and a refused key at lanes 0, 31 and 63 of an otherwise valid wavefront (and with a
    second, untouched wavefront behind it): the odd item reads what it must, every neighbour keeps its 1.  Both kernels that call
    ecmult_lane walk it in lock step: the odd lane walks it with zero scalars."""
    _odd_lane_checks(engine, pool, edge)


def test_fused_form(pool, edge, golden, engine):
    """S2K_OPT_S2C_FUSED: host verification as one kernel instead of the default chain of two.  The same verdicts on the recorded items in
    every format combination, on the odd lanes, and over sub-range launches of 256 lanes; the commitment check is not affected."""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_S2C_FUSED, 1)
        for sf, pf, of in S.FORMAT_COMBINATIONS:
            a = _arrays(golden, sf, pf, of)
            got = _host(eng, a)
            assert np.array_equal(got, a["host"]), (a["fmt"], _names(a, got, a["host"]))
        _odd_lane_checks(eng, pool, edge)
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        for fmt in ((0, 0, 0), (2, 0, 0)):
            a = _arrays(_take(pool, 700, start=3), *fmt)
            assert np.array_equal(_host(eng, a), a["host"]), fmt
            d_c, d_h = _both_dev(eng, a)
            eng.sync()
            assert np.array_equal(d_c.cpu().numpy(), a["commit"]) and np.array_equal(d_h.cpu().numpy(), a["host"]), fmt
        eng.set_option(Engine.OPT_S2C_FUSED, 0)
        assert np.array_equal(_host(eng, a), a["host"])
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def _odd_lane_checks(engine, pool, edge):
    valid = [x for x in pool if x[7] == 1][:128]
    by_name = {x[0]: x for x in edge}
    odd = [by_name["s = 0"], by_name["s -> n - s"], by_name["r + 1"], by_name["opening with prefix 04"], by_name["public key unparsable"],
           by_name["all-zero opening object"], by_name["all-zero public-key object"]]
    assert [x[6:8] for x in odd] == [(1, 0), (1, 0), (0, 0), (0, 0), (1, 0), (0, 0), (1, 0)]
    for it in odd:
        fmt = {"obj_opening": (0, 0, 1), "obj_pubkey": (0, 1, 0)}.get(it[8], (0, 0, 0))
        for lane in (0, 31, 63):
            for n in (64, 128):
                items = list(valid[:n]); items[lane] = it
                a = _arrays(items, *fmt)
                assert a["n"] == n and a["host"].sum() == n - 1 and a["host"][lane] == 0 and a["commit"].sum() == n - 1 + it[6]
                got = _host(engine, a)
                assert np.array_equal(got, a["host"]), (it[0], lane, n, np.flatnonzero(got != a["host"])[:8])
                got = _commit(engine, a)
                assert np.array_equal(got, a["commit"]), (it[0], lane, n, np.flatnonzero(got != a["commit"])[:8])


def test_host_commit_against_hashlib(engine):
    import torch
    t = hashlib.sha256(S.TAG_DATA).digest()
    rng = np.random.default_rng(5611)
    for n in (1, 64, 257):
        rnd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        rnd[0] = 0xFF
        want = np.frombuffer(b"".join(hashlib.sha256(t + t + rnd[i].tobytes()).digest() for i in range(n)), np.uint8).reshape(n, 32)
        assert np.array_equal(engine.anti_exfil_host_commit_batch(rnd), want), n
        d_out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
        engine.anti_exfil_host_commit_batch_dev(d_out, _dev(rnd))
        engine.sync()
        assert np.array_equal(d_out.cpu().numpy(), want), n
    for rnd, cm in json.load(open(os.path.join(HERE, "golden", "s2c_vectors.json")))["host_commit"]:
        assert engine.anti_exfil_host_commit_batch(bytes.fromhex(rnd)).tobytes().hex() == cm


def test_x_above_n_primitive_on_the_device(engine):
    """s2c_x_matches through tests/gpu_prims/s2c_prims.hip where no entry point takes it: x(R) = n + k with r = k and r = k + 1"""
    import torch
    path = os.path.join(HERE, "gpu_prims", "libs2k_s2c_prims.so")
    assert os.path.exists(path), "tests/gpu_prims/libs2k_s2c_prims.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.s2k_test_s2c_x_matches.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int]
    cases = S.x_above_n_cases() * 3                                                       # 84 lanes: a full wavefront and a partial one
    n = len(cases)
    col = lambda k, w: _dev(np.frombuffer(b"".join(c[k] for c in cases), np.uint8).reshape(n, w).copy())      # noqa: E731
    d_xy, d_z, d_r = col(1, 64), col(2, 32), col(3, 32)
    d_out = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.s2k_test_s2c_x_matches(d_out.data_ptr(), d_xy.data_ptr(), d_z.data_ptr(), d_r.data_ptr(), n) == 1
    got = d_out.cpu().numpy()
    want = np.array([c[4] for c in cases], np.int32)
    assert want.sum() == 36 and np.array_equal(got, want), [c[0] for c, g_, w in zip(cases, got, want) if g_ != w]
