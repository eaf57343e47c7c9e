"""GPU: MuSig2 key aggregation, cache tweaks, nonce aggregation and signature aggregation (csrc/musig_agg.h,
csrc/engine_musig_agg.hip).  Expected values are the reference's own where they are recorded (tests/golden/musig_agg_vectors.json)
and the Python model's (tests/musig_agg_ref.py, which agrees with the reference on every recorded row) elsewhere; the reference itself
is not needed."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import musig_agg_ref as A
from tests import musig_ref as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_IN = (A.KEYAGG_INPUTS, A.TWEAK_INPUTS, A.NONCE_INPUTS, A.SIG_INPUTS)
NAMES = ("keyagg", "tweak", "nonce_agg", "sig_agg")
NONCE_BYTES = {0: 66, 1: 132}
SIG_BYTES = {0: 32, 1: 36}
SET_SIZES = (1, 63, 64, 65, 257, 1000)


@pytest.fixture(scope="module")
def golden():
    j = json.load(open(os.path.join(HERE, "golden", "musig_agg_vectors.json")))
    return tuple(A.from_json(j[NAMES[w]], w, N_IN[w]) for w in range(4))


@pytest.fixture(scope="module")
def pool():
    """64 seeded key sets, every fourth with a flipped bit (tests/musig_agg_ref.py: keyagg_pool); computed once, never changed"""
    p = A.keyagg_pool()
    assert all(x[3][0] == 1 for x in p)                                                        # every uncorrupted set is served
    assert sum(1 for x in p if x[1] and x[2][0] == 0) >= 4                                      # corrupted: at least 4 refused,
    assert sum(1 for x in p if x[1] and x[2][0] == 1 and x[2][1] != x[3][1]) >= 4               # at least 4 served with another cache
    return p


def _np(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to("cuda:0")


def _filled(n, dtype=None):
    import torch
    return torch.full((max(n, 1),), 0xEE, dtype=dtype or torch.uint8, device="cuda:0")


def _side_stream():
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    return s, ctypes.c_void_p(s.cuda_stream)


def _off(blobs, size):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) // size for b in blobs])
    return off


def _cut(buf, k, w):
    return bytes(buf[w * k:w * k + w])


def _keyagg(engine, sets, f, dev=False):
    """[(verdict, cache, agg_pk)] of a batch of key blobs"""
    import torch
    n, off, blob = len(sets), _off(sets, A.PK_BYTES[f]), b"".join(sets)
    if dev:
        s, st = _side_stream()
        d_res, d_c, d_a = _filled(n, torch.int32), _filled(197 * n), _filled(64 * n)
        with torch.cuda.stream(s):
            engine.musig_pubkey_agg_dev(d_res, d_c, d_a, _dev(_np(blob)), off, pk_format=f, stream=st)
        s.synchronize()
        res, c, a = d_res.cpu().numpy()[:n], d_c.cpu().numpy(), d_a.cpu().numpy()
    else:
        res, c, a = engine.musig_pubkey_agg(_np(blob), off, pk_format=f)
    return [(int(res[k]), _cut(c, k, 197), _cut(a, k, 64)) for k in range(n)]


def _tweak(engine, rows, dev=False, in_place=False):
    import torch
    n = len(rows)
    caches, tweaks, xo = _np(b"".join(r[1] for r in rows)), _np(b"".join(r[2] for r in rows)), np.array([r[3] for r in rows], np.uint8)
    if dev:
        s, st = _side_stream()
        d_in = _dev(caches)
        d_res, d_c, d_p = _filled(n, torch.int32), (d_in if in_place else _filled(197 * n)), _filled(64 * n)
        with torch.cuda.stream(s):
            engine.musig_pubkey_tweak_add_dev(d_res, d_c, d_p, d_in, _dev(tweaks), _dev(xo), n=n, stream=st)
        s.synchronize()
        res, c, p = d_res.cpu().numpy(), d_c.cpu().numpy(), d_p.cpu().numpy()
    else:
        res, c, p = engine.musig_pubkey_tweak_add(caches, tweaks, xo)
    return [(int(res[k]), _cut(c, k, 197), _cut(p, k, 64)) for k in range(n)]


def _nonce_agg(engine, blobs, nf, of, dev=False):
    import torch
    n, off, blob = len(blobs), _off(blobs, NONCE_BYTES[nf]), b"".join(blobs)
    if dev:
        s, st = _side_stream()
        d_res, d_o = _filled(n, torch.int32), _filled(NONCE_BYTES[of] * n)
        with torch.cuda.stream(s):
            engine.musig_nonce_agg_dev(d_res, d_o, _dev(_np(blob)), off, nonce_format=nf, out_format=of, stream=st)
        s.synchronize()
        res, o = d_res.cpu().numpy(), d_o.cpu().numpy()
    else:
        res, o = engine.musig_nonce_agg(_np(blob), off, nonce_format=nf, out_format=of)
    return [(int(res[k]), _cut(o, k, NONCE_BYTES[of])) for k in range(n)]


def _sig_agg(engine, sessions, blobs, sf, dev=False):
    import torch
    n, off, blob = len(blobs), _off(blobs, SIG_BYTES[sf]), b"".join(blobs)
    if dev:
        s, st = _side_stream()
        d_res, d_o = _filled(n, torch.int32), _filled(64 * n)
        with torch.cuda.stream(s):
            engine.musig_partial_sig_agg_dev(d_res, d_o, _dev(_np(b"".join(sessions))), _dev(_np(blob)), off, sig_format=sf, stream=st)
        s.synchronize()
        res, o = d_res.cpu().numpy(), d_o.cpu().numpy()
    else:
        res, o = engine.musig_partial_sig_agg(_np(b"".join(sessions)), _np(blob), off, sig_format=sf)
    return [(int(res[k]), _cut(o, k, 64)) for k in range(n)]


def _check(got, want, names, what):
    assert len(got) == len(want)
    for g, w, nm in zip(got, want, names):
        assert g == tuple(w), (what, nm, g[0], w[0])


def _all_calls(engine, rows, dev):
    """every row of the four lists, one batch per format combination"""
    K, T, Nn, S = rows
    for f in range(3):
        kk = [r for r in K if r[1 + f] is not None]
        _check(_keyagg(engine, [r[1 + f] for r in kk], f, dev), [r[4:] for r in kk], [r[0] for r in kk], "keyagg format %d" % f)
    _check(_tweak(engine, T, dev), [r[4:] for r in T], [r[0] for r in T], "tweak")
    for nf in range(2):
        nn = [r for r in Nn if r[1 + nf] is not None]
        for of in range(2):
            _check(_nonce_agg(engine, [r[1 + nf] for r in nn], nf, of, dev), [(r[3], r[4 + of]) for r in nn], [r[0] for r in nn], "nonce_agg %d -> %d" % (nf, of))
    for sf in range(2):
        ss = [r for r in S if r[2 + sf] is not None]
        _check(_sig_agg(engine, [r[1] for r in ss], [r[2 + sf] for r in ss], sf, dev), [r[4:] for r in ss], [r[0] for r in ss], "sig_agg format %d" % sf)


def test_golden_one_batch_per_format(engine, golden):
    """every recorded row -- the module's BIP-327 vectors, the edge lists, the seeded rows -- against the reference's recorded answers"""
    _all_calls(engine, golden, dev=False)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_edge_lists(engine, dev):
    """the edge lists through the host form and through the _dev form on a caller's stream, into outputs pre-filled with 0xEE"""
    edges = (A.keyagg_edges(), A.tweak_edges(), A.nonce_edges(), A.sig_edges())
    _all_calls(engine, edges, dev)
    T = A.tweak_edges()
    _check(_tweak(engine, T, dev=True, in_place=True), [r[4:] for r in T], [r[0] for r in T], "tweak in place")
    # an empty set between two served ones; without the x-only output; xonly NULL
    K = {r[0]: r for r in A.keyagg_edges()}
    trio = [K["two keys (the second's coefficient is 1)"], K["an empty set"], K["[P, Q, Q]"]]
    _check(_keyagg(engine, [r[1] for r in trio], 0, dev), [r[4:] for r in trio], [r[0] for r in trio], "empty set between served ones")
    res, c, a = engine.musig_pubkey_agg(_np(trio[0][1]), np.array([0, 2], np.uint64), pk_format=0, want_agg_pk=False)
    assert a is None and (int(res[0]), bytes(c)) == tuple(trio[0][4:6])
    plain = [r for r in T if r[3] == 0]
    res, c, p = engine.musig_pubkey_tweak_add(_np(b"".join(r[1] for r in plain)), _np(b"".join(r[2] for r in plain)), None)
    assert [(int(res[k]), _cut(c, k, 197), _cut(p, k, 64)) for k in range(len(plain))] == [tuple(r[4:]) for r in plain]


@pytest.mark.parametrize("fanin", [2, 3])
def test_fanin_walk(engine, fanin):
    """set sizes 2..9 (up to four passes), 63..130 and the nonce edges at a small fan-in: results never depend on it"""
    from secp256k1_zkp_amd import Engine
    K, Nn = A.keyagg_edges(), A.nonce_edges()
    engine.set_option(Engine.OPT_MUSIG_SUM_FANIN, fanin)
    try:
        for f in (0, 1):
            _check(_keyagg(engine, [r[1 + f] for r in K if r[1 + f] is not None], f, dev=(f == 1)), [r[4:] for r in K if r[1 + f] is not None],
                   [r[0] for r in K if r[1 + f] is not None], "keyagg fan-in %d" % fanin)
        nn = [r for r in Nn if r[1] is not None]
        _check(_nonce_agg(engine, [r[1] for r in nn], 0, 0), [(r[3], r[4]) for r in nn], [r[0] for r in nn], "nonce_agg fan-in %d" % fanin)
    finally:
        engine.set_option(Engine.OPT_MUSIG_SUM_FANIN, 64)
    for bad in (1, 65, 0):
        with pytest.raises(Exception):
            engine.set_option(Engine.OPT_MUSIG_SUM_FANIN, bad)


def _term_key(lane, m):
    """the flat key that lane `lane` of a stage (b) launch of m keys takes (engine_musig_agg.hip: k_musig_agg_term)"""
    half = (m + 1) // 2
    return 2 * lane if lane < half else 2 * (lane - half) + 1


def _cyclic(pool, n):
    return [pool[i % len(pool)] for i in range(n)]


@pytest.mark.parametrize("fanin", [64, 2])
def test_sets_straddle_launch_boundaries(engine, pool, fanin):
    """about 700 keys in sets of 1..9 under S2K_OPT_MAX_LANES = 256: three key launches, sets cut by their boundaries"""
    from secp256k1_zkp_amd import Engine
    items, keys = [], 0
    while keys < 700:
        items.append(pool[len(items) % len(pool)]); keys += len(items[-1][0]) // 33
    off = _off([x[0] for x in items], 33)
    assert any(int(off[k]) < b < int(off[k + 1]) for b in (256, 512) for k in range(len(items)))        # a set really straddles each boundary
    engine.set_option(Engine.OPT_MAX_LANES, 256); engine.set_option(Engine.OPT_MUSIG_SUM_FANIN, fanin)
    try:
        _check(_keyagg(engine, [x[0] for x in items], 0, dev=True), [x[2] for x in items], range(len(items)), "MAX_LANES 256")
    finally:
        engine.set_option(Engine.OPT_MAX_LANES, 1 << 20); engine.set_option(Engine.OPT_MUSIG_SUM_FANIN, 64)


def test_refused_lanes_of_valid_wavefronts(engine, pool):
    """refused sets at set lanes 0, 31 and 63, and refused keys at key lanes 0, 31 and 63, of otherwise valid wavefronts; refused tweaks,
    nonce sessions and signature sessions at the same lanes"""
    _, pts = A._edge_points()
    bad = b"\x02" + M.b32(A.off_curve_x(pts[0][0]))
    good = [x for x in pool if not x[1]]
    sets = [good[i % len(good)][0] for i in range(64)]
    for lane in (0, 31, 63):
        sets[lane] = sets[lane][:-33] + bad                                                     # the set's last key does not parse
    got = _keyagg(engine, sets, 0)
    for k in range(64):
        assert got[k] == (A.NO_KEYAGG if k in (0, 31, 63) else good[k % len(good)][2]), k
    # Stage (b) does NOT run flat key i on lane i: k_musig_agg_term gives the first half of a launch the even keys and the second half the
    # odd ones.  The refused keys are therefore chosen through that map.  128 two-key sets: wavefronts 0 and 1 hold first keys (they
    # multiply), 2 and 3 second keys (coefficient 1: nothing to multiply).  64 three-key sets: every wavefront mixes both kinds.
    for size, n_sets, waves in ((2, 128, (0, 3)), (3, 64, (0, 2))):
        keys = [[M.ser33(pts[(i + j * (1 + i // 8 % 3)) % 10]) for j in range(size)] for i in range(n_sets)]
        assert all(len(set(ks)) == size for ks in keys)
        want = [A.keyagg_bytes(b"".join(ks), 0) for ks in keys]
        assert all(w[0] == 1 for w in want)
        for lane in [64 * w + x for w in waves for x in (0, 31, 63)]:
            key = _term_key(lane, size * n_sets)
            keys[key // size][key % size] = bad
            want[key // size] = A.NO_KEYAGG
        assert sum(w[0] == 0 for w in want) >= 5                                                # (two of the six lanes may share a set)
        assert _keyagg(engine, [b"".join(ks) for ks in keys], 0, dev=True) == want
    # one cache, one session per lane: a refused item at lanes 0, 31 and 63 of tweaks, nonce aggregation and signature aggregation
    T = [r for r in A.tweak_edges() if r[4] == 1]
    rows = [T[i % len(T)] for i in range(64)]
    for lane in (0, 31, 63):
        rows[lane] = A.make_trow("refused", rows[lane][1], M.b32(M.N), rows[lane][3])
    _check(_tweak(engine, rows, dev=True), [r[4:] for r in rows], range(64), "tweak lanes")
    Nn = [r for r in A.nonce_edges() if r[3] == 1 and len(r[1]) <= 4 * 66]
    rows = [Nn[i % len(Nn)] for i in range(64)]
    for lane in (0, 31, 63):
        rows[lane] = A.make_nrow("refused", ser=rows[lane][1][:-33] + bad)                      # the last point does not parse
    assert all(rows[k][3] == (0 if k in (0, 31, 63) else 1) for k in range(64))
    _check(_nonce_agg(engine, [r[1] for r in rows], 0, 0, dev=True), [(r[3], r[4]) for r in rows], range(64), "nonce_agg lanes")
    S = [r for r in A.sig_edges() if r[4] == 1 and r[2] is not None]
    rows = [S[i % len(S)] for i in range(64)]
    for lane in (0, 31, 63):
        rows[lane] = A.make_srow("refused", rows[lane][1], ser=rows[lane][2][:-32] + M.b32(M.N))   # the last share is not below n
    assert all(rows[k][4] == (0 if k in (0, 31, 63) else 1) for k in range(64))
    _check(_sig_agg(engine, [r[1] for r in rows], [r[2] for r in rows], 0, dev=True), [r[4:] for r in rows], range(64), "sig_agg lanes")


@pytest.mark.parametrize("n", SET_SIZES)
def test_batch_sizes(engine, pool, n):
    """n sets cut cyclically from the pool, through the _dev form"""
    items = _cyclic(pool, n)
    _check(_keyagg(engine, [x[0] for x in items], 0, dev=True), [x[2] for x in items], range(n), "%d sets" % n)


def test_single_item_form(engine, golden):
    from secp256k1_zkp_amd import _native
    lib = _native.load()
    r = next(r for r in golden[0] if r[0] == "BIP-327 key_agg valid 0")
    objs = [ctypes.create_string_buffer(k, 64) for k in A.split(r[2], 64)]
    arr = (ctypes.c_void_p * len(objs))(*[ctypes.addressof(o) for o in objs])
    cache, agg = ctypes.create_string_buffer(197), ctypes.create_string_buffer(b"\xee" * 64, 64)
    assert lib.secp256k1_musig_pubkey_agg_amd(None, agg, cache, arr, len(objs)) == 1 and (cache.raw, agg.raw) == (r[5], r[6])
    assert lib.secp256k1_musig_pubkey_agg_amd(None, None, None, arr, len(objs)) == 1
    objs[1] = ctypes.create_string_buffer(64); arr[1] = ctypes.addressof(objs[1])              # an all-zero key object
    assert lib.secp256k1_musig_pubkey_agg_amd(None, agg, cache, arr, len(objs)) == 0 and agg.raw == bytes(64)


def test_signing_round_on_one_stream(engine):
    """16 sessions x 3 signers, entirely through _dev calls on one stream: pubkey_agg -> x-only tweak (in place) -> nonce_agg ->
    nonce_process -> partial_sig_verify (session_of) -> partial_sig_agg -> BIP-340 verification of the 16 final signatures under the x
    coordinate of the tweaked key.  Every fourth session carries one corrupted share: its verdict is 0 and that session's signature
    does not verify; every intermediate array equals the model's."""
    import torch
    rng = np.random.default_rng(6627)
    ns, m = 16, 3
    tw = [M._rand_scalar(rng) for _ in range(ns)]
    scs = [M.Scenario(rng, [M._rand_scalar(rng) for _ in range(m)], tweaks=[(tw[k], 1)]) for k in range(ns)]
    shares = [[sc.share(j) for j in range(m)] for sc in scs]
    corrupted = [(k, k % m) for k in range(ns) if k % 4 == 3]
    for k, j in corrupted:
        shares[k][j] = (shares[k][j] + 1) % M.N
    keys = b"".join(M.ser33(p) for sc in scs for p in sc.pks)
    nonces = b"".join(M.pubnonce_ser(*r) for sc in scs for r in sc.Rs)
    sigs = b"".join(M.b32(s) for row in shares for s in row)
    off = np.arange(0, ns * m + 1, m, dtype=np.uint64)
    d_keys, d_nonces, d_sigs = _dev(_np(keys)), _dev(_np(nonces)), _dev(_np(sigs))
    d_tw, d_xo, d_msgs = _dev(_np(b"".join(M.b32(t) for t in tw))), _dev(np.ones(ns, np.uint8)), _dev(_np(b"".join(sc.msg for sc in scs)))
    d_of = _dev(np.repeat(np.arange(ns, dtype=np.int32), m))
    i32 = torch.int32
    r1, r2, r3, r4, r5, r6, r7 = (_filled(ns, i32), _filled(ns, i32), _filled(ns, i32), _filled(ns, i32), _filled(ns * m, i32), _filled(ns, i32), _filled(ns, i32))
    d_cache0, d_cache, d_agg, d_pk, d_an, d_sess, d_sig64 = _filled(197 * ns), _filled(197 * ns), _filled(64 * ns), _filled(64 * ns), _filled(66 * ns), _filled(133 * ns), _filled(64 * ns)
    s, st = _side_stream()
    with torch.cuda.stream(s):
        engine.musig_pubkey_agg_dev(r1, d_cache0, d_agg, d_keys, off, stream=st)
        d_cache.copy_(d_cache0)
        engine.musig_pubkey_tweak_add_dev(r2, d_cache, d_pk, d_cache, d_tw, d_xo, n=ns, stream=st)
        engine.musig_nonce_agg_dev(r3, d_an, d_nonces, off, stream=st)
        engine.musig_nonce_process_dev(r4, d_sess, d_an, d_msgs, d_cache, stream=st)
        engine.musig_partial_sig_verify_dev(r5, d_sigs, d_nonces, d_keys, d_cache, d_sess, ns, session_of=d_of, stream=st)
        engine.musig_partial_sig_agg_dev(r6, d_sig64, d_sess, d_sigs, off, stream=st)
        d_x = torch.flip(d_pk.view(ns, 64)[:, :32], dims=[1]).contiguous()                      # the object's x is little-endian
        engine.schnorrsig_verify_batch_dev(r7, d_sig64, d_msgs, d_x, stream=st)
    s.synchronize()
    for r in (r1, r2, r3, r4, r6):
        assert r.cpu().tolist() == [1] * ns
    assert bytes(d_cache0.cpu().numpy()) == b"".join(M.pubkey_agg(sc.pks) for sc in scs)
    assert bytes(d_cache.cpu().numpy()) == b"".join(sc.cache for sc in scs)
    assert bytes(d_pk.cpu().numpy()) == b"".join(sc.cache[4:68] for sc in scs)
    assert bytes(d_an.cpu().numpy()) == b"".join(M.aggnonce_ser(*sc.agg) for sc in scs)
    assert bytes(d_sess.cpu().numpy()) == b"".join(sc.session for sc in scs)
    verdicts = np.ones((ns, m), np.int32)
    for k, j in corrupted:
        verdicts[k, j] = 0
    assert r5.cpu().tolist() == verdicts.reshape(-1).tolist()
    assert bytes(d_sig64.cpu().numpy()) == b"".join(A.partial_sig_agg(scs[k].session, shares[k]) for k in range(ns))
    assert r7.cpu().tolist() == [0 if k % 4 == 3 else 1 for k in range(ns)]
