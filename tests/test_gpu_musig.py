"""GPU: MuSig2 partial-signature verification and nonce processing (csrc/musig.h, csrc/engine_musig.hip).  The verdicts and sessions
are the reference's own where they are recorded (tests/golden/musig_vectors.json) and the Python model's (tests/musig_ref.py, which
agrees with the reference on every recorded row) elsewhere; the reference itself is not needed."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import musig_ref as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIG_BYTES = {0: 32, 1: 36}
NONCE_BYTES = {0: 66, 1: 132}
KEY_BYTES = {0: 33, 1: 64, 2: 65}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
PROCESS_SIZES = (1, 64, 65, 257, 1000)


@pytest.fixture(scope="module")
def golden():
    j = json.load(open(os.path.join(HERE, "golden", "musig_vectors.json")))
    return M.from_json(j["verify"], M.VERIFY_INPUTS), M.from_json(j["process"], M.PROCESS_INPUTS)


@pytest.fixture(scope="module")
def edge():
    return M.edge_cases()


@pytest.fixture(scope="module")
def pool():
    """200 seeded shares on eight sessions, one in eight corrupted; the batches below are cut from it (cyclically for the largest)"""
    caches, sessions, items = M.shared_pool(200, 6610)
    assert sum(x[4] for x in items) == 175                                                # every uncorrupted share is valid, every flipped bit fatal
    return caches, sessions, items


@pytest.fixture(scope="module")
def ppool():
    items = M.process_pool(100, 6611)
    assert 80 <= sum(x[4][0] for x in items) < 100
    return items


def _u8(bs, w):
    return np.frombuffer(b"".join(bs), np.uint8).reshape(len(bs), w).copy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(rows, f):
    """verify rows that exist in the format combination f, one pair per row -> (kept, sigs, nonces, pks, caches, sessions, expected)"""
    kept, a = [], []
    for r in rows:
        x = M.verify_formats(r, *f)
        if x is not None:
            kept.append(r); a.append(x)
    return (kept, _u8([x[0] for x in a], SIG_BYTES[f[0]]), _u8([x[1] for x in a], NONCE_BYTES[f[1]]), _u8([x[2] for x in a], KEY_BYTES[f[2]]),
            _u8([r[7] for r in kept], 197), _u8([r[8] for r in kept], 133), np.array([r[9] for r in kept], np.int32))


def _fmt(f):
    return dict(sig_format=f[0], nonce_format=f[1], pk_format=f[2])


def _names(items, got, exp):
    return [x[0] for x, g, e in zip(items, got, exp) if g != e]


def _prows(rows, nf, adaptor):
    """process rows in nonce format nf, with (True) or without (False) an adaptor"""
    kept = [r for r in rows if M.process_formats(r, nf) is not None and (r[5] is not None) == adaptor]
    return (kept, _u8([M.process_formats(r, nf) for r in kept], NONCE_BYTES[nf]), _u8([r[3] for r in kept], 32), _u8([r[4] for r in kept], 197),
            _u8([r[5] for r in kept], 64) if adaptor else None, np.array([r[6] for r in kept], np.int32), _u8([r[7] for r in kept], 133))


def _check_process(engine, rows, nf, adaptor, dev=False, stream=None):
    import torch
    kept, nonces, msgs, caches, ads, exp, exp_sess = _prows(rows, nf, adaptor)
    if dev:
        n = len(kept)
        d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_out = torch.full((n, 133), 0xEE, dtype=torch.uint8, device="cuda:0")
        engine.musig_nonce_process_dev(d_res, d_out, _dev(nonces), _dev(msgs), _dev(caches), adaptors=None if ads is None else _dev(ads), nonce_format=nf, stream=stream)
        torch.cuda.synchronize()
        got, sess = d_res.cpu().numpy(), d_out.cpu().numpy()
    else:
        got, sess = engine.musig_nonce_process(nonces, msgs, caches, adaptors=ads, nonce_format=nf)
        sess = sess.reshape(-1, 133)
    assert np.array_equal(got, exp), (nf, adaptor, _names(kept, got, exp))
    assert np.array_equal(sess, exp_sess), (nf, adaptor, [kept[i][0] for i in np.flatnonzero((sess != exp_sess).any(axis=1))])
    return len(kept)


def test_golden_fixture_one_batch_per_format(engine, golden):
    """every recorded row in one batch per format combination: the reference's verdicts and sessions"""
    V, Pr = golden
    for f in M.ALL_VERIFY_FORMATS:
        kept, sigs, nonces, pks, caches, sessions, exp = _rows(V, f)
        assert len(kept) >= 0.8 * len(V) and 0 < exp.sum() < len(kept)
        got = engine.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, **_fmt(f))
        assert np.array_equal(got, exp), (f, _names(kept, got, exp))
    ran = sum(_check_process(engine, Pr, nf, adaptor) for nf in (0, 1) for adaptor in (False, True))
    assert ran >= 1.6 * len(Pr)                                                           # both nonce formats, each at least 80 % of the rows


def test_verify_edge_list_host_dev_group_amd(engine, edge):
    """the verify edge list through the host and _dev forms (the latter on a caller's stream, into results pre-filled with 7), through a
    group of one engine, and item by item through the _amd form (objects)"""
    import torch
    from secp256k1_zkp_amd import Group
    V = edge[0]
    g = Group([0])
    s = torch.cuda.Stream()
    try:
        for f in ((0, 0, 0), (1, 1, 1), (0, 1, 2), (1, 0, 0)):
            kept, sigs, nonces, pks, caches, sessions, exp = _rows(V, f)
            assert len(kept) >= 30 and 0 < exp.sum() < len(kept)                      # (the edge list is dense in rows only one representation can express)
            got = engine.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, **_fmt(f))
            assert np.array_equal(got, exp), (f, _names(kept, got, exp))
            s.wait_stream(torch.cuda.current_stream())
            d_res = torch.full((len(kept),), 7, dtype=torch.int32, device="cuda:0")
            engine.musig_partial_sig_verify_dev(d_res, _dev(sigs), _dev(nonces), _dev(pks), _dev(caches), _dev(sessions), len(kept), stream=ctypes.c_void_p(s.cuda_stream), **_fmt(f))
            s.synchronize()
            got = d_res.cpu().numpy()
            assert np.array_equal(got, exp), (f, _names(kept, got, exp))
            got = g.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, **_fmt(f))
            assert np.array_equal(got, exp), (f, _names(kept, got, exp))
        L = engine._lib
        kept, sigs, nonces, pks, caches, sessions, exp = _rows(V, (1, 1, 1))
        assert {"wrong magic: partial signature", "wrong magic: pubnonce", "all-zero key object", "object s = n, valid as 0"} <= {r[0] for r in kept}
        for r in kept:
            assert L.secp256k1_musig_partial_sig_verify_amd(None, r[2], r[4], r[6], r[7], r[8]) == r[9] and L.s2k_last_status() == 0, r[0]
    finally:
        g.close()


def test_process_edge_list_host_dev(engine, edge):
    """the process edge list through the host and _dev forms, sessions byte for byte (133 zero bytes where the verdict is 0)"""
    import torch
    s = torch.cuda.Stream()
    ran = 0
    for nf in (0, 1):
        for adaptor in (False, True):
            ran += _check_process(engine, edge[1], nf, adaptor)
            s.wait_stream(torch.cuda.current_stream())
            _check_process(engine, edge[1], nf, adaptor, dev=True, stream=ctypes.c_void_p(s.cuda_stream))
    assert ran >= 2 * len(edge[1]) - 3                                                    # three rows exist in one representation only


def _cut(pool, n, start=0):
    caches, sessions, items = pool
    it = [items[(start + i) % len(items)] for i in range(n)]
    return (it, _u8([x[0] for x in it], 32), _u8([x[1] for x in it], 66), _u8([x[2] for x in it], 33), np.array([x[3] for x in it], np.uint32),
            np.array([x[4] for x in it], np.int32))


def test_verify_batch_sizes(engine, pool):
    """1 .. 1000 shares, one in eight corrupted, on eight sessions shared through session_of; then one pair per share (session_of NULL)"""
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    for n in SIZES:
        it, sigs, nonces, pks, of, exp = _cut(pool, n, start=n)
        assert n < 8 or 0 < exp.sum() < n
        got = engine.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=of)
        assert np.array_equal(got, exp), (n, np.flatnonzero(got != exp)[:8])
        got = engine.musig_partial_sig_verify(sigs, nonces, pks, caches[of], sessions[of])
        assert np.array_equal(got, exp), (n, "one pair per share", np.flatnonzero(got != exp)[:8])


def test_process_batch_sizes(engine, ppool):
    """1 .. 1000 items with and without adaptors; the sessions byte for byte"""
    for n in PROCESS_SIZES:
        it = [ppool[(n + i) % len(ppool)] for i in range(n)]
        nonces, msgs, caches, ads = _u8([x[0] for x in it], 66), _u8([x[1] for x in it], 32), _u8([x[2] for x in it], 197), _u8([x[3] for x in it], 64)
        for k, a in ((4, None), (5, ads)):
            got, sess = engine.musig_nonce_process(nonces, msgs, caches, adaptors=a)
            assert np.array_equal(got, np.array([x[k][0] for x in it], np.int32)), (n, k)
            assert np.array_equal(sess.reshape(n, 133), _u8([x[k][1] for x in it], 133)), (n, k)


def test_sub_range_launches(engine, pool, ppool):
    """700 items on an engine whose launches take 256 and then 512 lanes: sub-range launches, equal to the single-launch results, with
    the pairs shared through session_of and with one pair per share (the pair arrays then move with the sub-range)"""
    import torch
    from secp256k1_zkp_amd import Engine
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    it, sigs, nonces, pks, of, exp = _cut(pool, 700, start=3)
    one = engine.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=of)
    assert np.array_equal(one, exp) and 0 < exp.sum() < 700
    pit = [ppool[i % len(ppool)] for i in range(700)]
    pn, pm, pc, pa = _u8([x[0] for x in pit], 66), _u8([x[1] for x in pit], 32), _u8([x[2] for x in pit], 197), _u8([x[3] for x in pit], 64)
    pone = engine.musig_nonce_process(pn, pm, pc, adaptors=pa)
    assert np.array_equal(pone[1].reshape(700, 133), _u8([x[5][1] for x in pit], 133))
    eng = Engine(0)
    try:
        for lanes in (256, 512):
            eng.set_option(Engine.OPT_MAX_LANES, lanes)
            assert np.array_equal(eng.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=of), one), lanes
            assert np.array_equal(eng.musig_partial_sig_verify(sigs, nonces, pks, caches[of], sessions[of]), one), lanes
            d_res = torch.full((700,), 7, dtype=torch.int32, device="cuda:0")
            eng.musig_partial_sig_verify_dev(d_res, _dev(sigs), _dev(nonces), _dev(pks), _dev(caches), _dev(sessions), 8, session_of=_dev(of.view(np.int32)))
            eng.sync()
            assert np.array_equal(d_res.cpu().numpy(), one), lanes
            got = eng.musig_nonce_process(pn, pm, pc, adaptors=pa)
            assert np.array_equal(got[0], pone[0]) and np.array_equal(got[1], pone[1]), lanes
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_one_odd_lane_in_a_valid_wavefront(engine, pool, edge, ppool):
    """a fallback item (a zero scalar drives the wavefront out of the lock-step joint form), a refused key and a wrong magic at lanes 0,
    31 and 63 of an otherwise valid wavefront, with a second, untouched wavefront behind it: every neighbour keeps its verdict.  For
    nonce processing: an item whose R1 is infinite, and one whose R1 + A is, among adaptor items (the shared first inversion)."""
    valid = [x for x in pool[2] if x[4] == 1][:128]
    by_name = {r[0]: r for r in edge[0]}
    for name in ("hand-made session with b = 0", "compressed key: prefix 04", "wrong magic: cache", "R2 = -P"):
        r = by_name[name]
        for lane in (0, 31, 63):
            for n in (64, 128):
                it = list(valid[:n])
                caches, sessions = list(pool[0]) + [r[7]], list(pool[1]) + [r[8]]
                it[lane] = (r[1], r[3], r[5], 8, r[9])
                exp = np.array([x[4] for x in it], np.int32)
                assert exp.sum() == n - 1 + r[9]
                got = engine.musig_partial_sig_verify(_u8([x[0] for x in it], 32), _u8([x[1] for x in it], 66), _u8([x[2] for x in it], 33), _u8(caches, 197),
                                                      _u8(sessions, 133), session_of=np.array([x[3] for x in it], np.uint32))
                assert np.array_equal(got, exp), (name, lane, n, np.flatnonzero(got != exp)[:8])
    good = [x for x in ppool if x[5][0] == 1][:64]
    pe = {r[0]: r for r in edge[1]}
    for name in ("adaptor on an infinite R1", "adaptor = -R1", "adaptor = R1 (the doubling)", "all-zero adaptor object"):
        r = pe[name]
        for lane in (0, 31, 63):
            it = [(x[0], x[1], x[2], x[3], x[5]) for x in good]
            it[lane] = (r[1], r[3], r[4], r[5], (r[6], r[7]))
            got, sess = engine.musig_nonce_process(_u8([x[0] for x in it], 66), _u8([x[1] for x in it], 32), _u8([x[2] for x in it], 197), adaptors=_u8([x[3] for x in it], 64))
            assert np.array_equal(got, np.array([x[4][0] for x in it], np.int32)), (name, lane)
            assert np.array_equal(sess.reshape(64, 133), _u8([x[4][1] for x in it], 133)), (name, lane)


def test_chain_process_then_verify_on_one_stream(engine):
    """257 items: the sessions nonce_process_batch_dev writes are handed to partial_sig_verify_batch_dev on the same stream without a
    host copy; shares made by the model under those sessions verify, one flipped bit per eight items does not"""
    import torch
    items = M.chain_items(257, 6612)
    n = len(items)
    exp = np.array([x[6] for x in items], np.int32)
    assert exp.sum() == n - n // 8
    s = torch.cuda.Stream()
    d = [_dev(_u8([x[k] for x in items], w)) for k, w in ((0, 66), (1, 32), (2, 197), (3, 32), (4, 66), (5, 33))]
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_sess = torch.full((n, 133), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    s.wait_stream(torch.cuda.current_stream())
    st = ctypes.c_void_p(s.cuda_stream)
    engine.musig_nonce_process_dev(d_ok, d_sess, d[0], d[1], d[2], stream=st)
    engine.musig_partial_sig_verify_dev(d_res, d[3], d[4], d[5], d[2], d_sess, n, stream=st)
    s.synchronize()
    assert d_ok.cpu().numpy().all()
    got = d_res.cpu().numpy()
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]


def test_argument_checks(engine, pool):
    """NULL where the reference has ARG_CHECK and a format out of range fail the call with the argument status; an index >= n_sessions
    fails the host form and gives verdict 0 to that item alone in the _dev form; n == 0 succeeds"""
    import torch
    L = engine._lib; h = engine._h
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    it, sigs, nonces, pks, of, exp = _cut(pool, 6)
    assert exp.all()
    res = np.full(6, 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(sigs), 0, p(nonces), 0, p(pks), 0, p(caches), p(sessions), 8, p(of), 6]
    assert L.secp256k1_musig_partial_sig_verify_batch(h, *good) == 1 and np.array_equal(res, exp)
    for k in (0, 1, 3, 5, 7, 8):
        a = list(good); a[k] = None
        assert L.secp256k1_musig_partial_sig_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
        assert L.secp256k1_musig_partial_sig_verify_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, k
    for k, bad in ((2, 2), (2, -1), (4, 2), (4, -1), (6, 3), (6, -1)):
        a = list(good); a[k] = bad
        assert L.secp256k1_musig_partial_sig_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any(), (k, bad)
        assert L.secp256k1_musig_partial_sig_verify_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, (k, bad)
    a = list(good); a[10] = None                                                          # session_of NULL needs n_sessions == n
    assert L.secp256k1_musig_partial_sig_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2
    bad_of = of.copy(); bad_of[2] = 8
    a = list(good); a[10] = p(bad_of)
    assert L.secp256k1_musig_partial_sig_verify_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any()
    with pytest.raises(Exception):
        engine.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=bad_of)
    d_res = torch.full((6,), 7, dtype=torch.int32, device="cuda:0")
    engine.musig_partial_sig_verify_dev(d_res, _dev(sigs), _dev(nonces), _dev(pks), _dev(caches), _dev(sessions), 8, session_of=_dev(bad_of.view(np.int32)))
    engine.sync()
    assert d_res.cpu().numpy().tolist() == [1, 1, 0, 1, 1, 1]
    assert L.secp256k1_musig_partial_sig_verify_batch(h, None, None, 0, None, 0, None, 0, None, None, 0, None, 0) == 1
    assert L.secp256k1_musig_partial_sig_verify_batch_dev(h, None, None, None, 0, None, 0, None, 0, None, None, 0, None, 0) == 1
    # nonce processing
    out = np.full(133 * 6, 0xEE, np.uint8); msgs = np.zeros((6, 32), np.uint8); an = _u8([M.aggnonce_ser(M.G, M.G)] * 6, 66); pc = caches[of]
    goodp = [p(res), p(out), p(an), 0, p(msgs), p(pc), None, 6]
    assert L.secp256k1_musig_nonce_process_batch(h, *goodp) == 1 and res.all() and out.reshape(6, 133)[:, :4].tobytes() == M.MAGIC_SESSION * 6
    for k in (0, 1, 2, 4, 5):
        a = list(goodp); a[k] = None
        assert L.secp256k1_musig_nonce_process_batch(h, *a) == 0 and L.s2k_last_status() == 2, k
        assert L.secp256k1_musig_nonce_process_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, k
    for bad in (2, -1):
        a = list(goodp); a[3] = bad
        assert L.secp256k1_musig_nonce_process_batch(h, *a) == 0 and L.s2k_last_status() == 2 and not res.any() and not out.any(), bad
        assert L.secp256k1_musig_nonce_process_batch_dev(h, None, *a) == 0 and L.s2k_last_status() == 2, bad
    assert L.secp256k1_musig_nonce_process_batch(h, None, None, None, 0, None, None, None, 0) == 1
    assert L.secp256k1_musig_nonce_process_batch_dev(h, None, None, None, None, 0, None, None, None, 0) == 1
    assert engine.musig_partial_sig_verify(b"", b"", b"", b"", b"").size == 0
