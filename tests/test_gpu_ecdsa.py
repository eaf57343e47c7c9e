"""GPU tier: ECDSA batch verification and public-key recovery (csrc/engine_ecdsa.hip) against the unmodified reference
(oracle/_ref through tests/ecdsa_ref.py) and the Wycheproof fixture (tests/golden/ecdsa_wycheproof.json)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PK_BYTES = {0: 33, 1: 64, 2: 65}


@pytest.fixture(scope="module")
def eref(ref):
    from tests.ecdsa_ref import EcdsaRef
    return EcdsaRef()


@pytest.fixture(scope="module")
def batch(eref):
    """4 096 reference-made signatures, made once for the module"""
    return eref.make(4096, np.random.default_rng(2201))


@pytest.fixture(scope="module")
def rec(eref):
    return eref.make_recoverable(4096, np.random.default_rng(2202))


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda:0")


def _verify_dev(engine, sigs, sig_format, msgs, pks, pk_format):
    """the same batch through secp256k1_ecdsa_verify_batch_dev: every array a torch tensor on cuda:0"""
    import torch
    from secp256k1_zkp_amd import Engine
    if sig_format == 2:
        data, off = Engine.pack([bytes(s) for s in sigs])
        n = len(sigs)
        d_sig = _dev(np.concatenate([data, np.zeros(8, np.uint8)])); d_off = _dev(off.astype(np.int64))
    else:
        n = sigs.shape[0]
        d_sig = _dev(sigs); d_off = None
    res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    d_msg, d_pk = _dev(msgs), _dev(pks)                          # (held until the engine's stream has drained)
    engine.ecdsa_verify_batch_dev(res, d_sig, d_msg, d_pk, sig_format=sig_format, pk_format=pk_format, sig_off=d_off, n=n)
    engine.sync()
    return res.cpu().numpy()


def test_wycheproof_and_edges_one_batch(engine, eref):
    """the 463 Wycheproof vectors and the DER / 65-byte-key part of the edge list in ONE batch (the 4 172-byte signature next to 8-byte
    ones), host form and device form"""
    from tests.test_cpu_ecdsa import wycheproof
    from tests.ecdsa_ref import edge_cases
    sigs, msgs, pks, exp, names = [], [], [], [], []
    for tc, key, h, sig, verdict in wycheproof():
        sigs.append(sig); msgs.append(h); pks.append(key); exp.append(verdict); names.append("wycheproof %d" % tc)
    assert max(len(s) for s in sigs) == 4172 and min(len(s) for s in sigs) <= 8
    cases = edge_cases(eref, np.random.default_rng(12))
    for name, sig, sf, msg, pk, pf, expected in cases:
        if sf == 2 and pf in (0, 2):                     # DER items go along in this batch, keys re-serialised to 65 bytes where they parse
            if pf == 0:
                o = eref.pubkey_parse(pk)
                if o is None:
                    continue
                pk = eref.pubkey_serialize(o, False)
            sigs.append(sig); msgs.append(msg); pks.append(pk); exp.append(expected); names.append(name)
    exp = np.array(exp, np.int32)
    M = np.frombuffer(b"".join(msgs), np.uint8).reshape(-1, 32); K = np.frombuffer(b"".join(pks), np.uint8).reshape(-1, 65)
    assert len(sigs) > 463 + 20 and exp.sum() >= 163
    got = engine.ecdsa_verify_batch(sigs, M, K, sig_format=2, pk_format=2)
    assert np.array_equal(got, exp), [names[i] for i in np.flatnonzero(got != exp)]
    got = _verify_dev(engine, sigs, 2, M, K, 2)
    assert np.array_equal(got, exp), [names[i] for i in np.flatnonzero(got != exp)]


def test_edge_list(engine, eref):
    """every item of the edge list in its own encoding: grouped by (sig_format, pk_format), one batch per group, host and device form"""
    from tests.ecdsa_ref import edge_cases
    cases = edge_cases(eref, np.random.default_rng(12))
    groups = {}
    for c in cases:
        groups.setdefault((c[2], c[5]), []).append(c)
    assert len(groups) >= 5
    for (sf, pf), items in groups.items():
        exp = np.array([c[6] for c in items], np.int32)
        sigs = [c[1] for c in items] if sf == 2 else np.frombuffer(b"".join(c[1] for c in items), np.uint8).reshape(-1, 64)
        M = np.frombuffer(b"".join(c[3] for c in items), np.uint8).reshape(-1, 32)
        K = np.frombuffer(b"".join(c[4] for c in items), np.uint8).reshape(-1, PK_BYTES[pf])
        got = engine.ecdsa_verify_batch(sigs, M, K, sig_format=sf, pk_format=pf)
        assert np.array_equal(got, exp), [items[i][0] for i in np.flatnonzero(got != exp)]
        got = _verify_dev(engine, sigs, sf, M, K, pf)
        assert np.array_equal(got, exp), [items[i][0] for i in np.flatnonzero(got != exp)]


def test_random_all_formats(engine, eref, batch):
    """4 096 random signatures x all nine encoding pairs, 1/16 corrupted, equal to the reference item by item"""
    from tests.ecdsa_ref import corrupt, der_encode
    n = 4096
    for sf in (0, 1, 2):
        for pf in (0, 1, 2):
            rng = np.random.default_rng(300 + 3 * sf + pf)
            msgs = batch["msgs"].copy(); pks = eref.pks_as(batch["pkobj"], pf)
            s64 = eref.sigs_as(batch["sigobj"], 0 if sf == 2 else sf)
            idx = corrupt(rng, s64, msgs, pks, 1 / 16)
            assert 180 <= len(idx) <= 340
            sigs = s64 if sf != 2 else [der_encode(int.from_bytes(s64[i, :32].tobytes(), "big"), int.from_bytes(s64[i, 32:].tobytes(), "big")) for i in range(n)]
            exp = eref.verify_many(sigs, sf, msgs, pks, pf)
            got = engine.ecdsa_verify_batch(sigs, msgs, pks, sig_format=sf, pk_format=pf)
            assert np.array_equal(got, exp), (sf, pf, np.flatnonzero(got != exp)[:8])
            ok = np.ones(n, bool); ok[idx] = False
            assert exp[ok].all() and n - len(idx) <= exp.sum() < n - len(idx) // 4
            if sf == 2 or pf == 2:
                assert np.array_equal(_verify_dev(engine, sigs, sf, msgs, pks, pf), exp), (sf, pf)


def test_full_size(engine, eref):
    """2^16 signatures, a fixed pseudo-random 1/256 corrupted (one bit of r or s), compact signatures and compressed keys"""
    rng = np.random.default_rng(2216)
    n = 1 << 16
    d = eref.make(n, rng)
    sigs = eref.sigs_as(d["sigobj"], 0); pks = eref.pks_as(d["pkobj"], 0); msgs = d["msgs"]
    bad = rng.choice(n, n // 256, replace=False)
    for k, i in enumerate(bad):
        sigs[i, (32 if k & 1 else 0) + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
    exp = eref.verify_many(sigs, 0, msgs, pks, 0)
    res = engine.ecdsa_verify_batch(sigs, msgs, pks)
    assert np.array_equal(res, exp) and exp.sum() == n - n // 256


def test_batch_sizes(eref, batch, rec):
    """1, 63, 64, 65, 255, 257 and max_lanes + 1 items (chunk boundary, partial last wavefront: the wave-shared inversion of the recovery
    kernel sees dead lanes), on an engine whose launches take 512 lanes"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 512)
        sigs = eref.sigs_as(batch["sigobj"][:1100], 0); pks = eref.pks_as(batch["pkobj"][:1100], 0); msgs = batch["msgs"][:1100].copy()
        sigs[::7, 40] ^= 1
        exp = eref.verify_many(sigs, 0, msgs, pks, 0)
        ders = [eref.sig_serialize_der(o) if o is not None else b"\x30\x00" for o in (eref.sig_parse_compact(sigs[i].tobytes()) for i in range(1100))]
        rm, rs, rid, rpk = (a[:1100].copy() for a in rec)
        rs[::5, 3] ^= 2
        rexp, rkeys = eref.recover_many(rs, rid, rm)
        assert 0 < exp.sum() < 1100 and 0 < rexp.sum() < 1100
        for n in (1, 63, 64, 65, 255, 257, 513, 1025, 1100):
            assert np.array_equal(eng.ecdsa_verify_batch(sigs[:n], msgs[:n], pks[:n]), exp[:n]), n
            assert np.array_equal(eng.ecdsa_verify_batch(ders[:n], msgs[:n], pks[:n], sig_format=2), exp[:n]), n
            got, keys = eng.ecdsa_recover_batch(rs[:n], rid[:n], rm[:n])
            assert np.array_equal(got, rexp[:n]) and np.array_equal(keys, rkeys[:n]), n
        assert eng.ecdsa_verify_batch(sigs[:0], msgs[:0], pks[:0]).size == 0
    finally:
        eng.close()


def test_recover(engine, eref, rec):
    """4 096 items over all four recids, 1/16 corrupted: verdicts and the 64 output bytes equal the reference's; recovered keys verify"""
    import torch
    from tests.ecdsa_ref import recover_cases
    rng = np.random.default_rng(2203)
    msgs, sigs, recids, pkobj = (a.copy() for a in rec)
    n = sigs.shape[0]
    got, keys = engine.ecdsa_recover_batch(sigs, recids, msgs)
    assert got.all() and np.array_equal(keys, pkobj)
    assert engine.ecdsa_verify_batch(sigs, msgs, keys, sig_format=0, pk_format=1).all()
    # every item under another recid, 1/16 with a flipped bit of r, s or the message, a few recid bytes out of range
    rid = ((recids.astype(np.int64) + np.arange(n) % 4) % 4).astype(np.uint8)
    bad = np.flatnonzero(rng.integers(0, 16, n) == 0)
    for k, i in enumerate(bad):
        if k % 3 == 2:
            msgs[i, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        else:
            sigs[i, 32 * (k % 3) + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
    rid[5::97] = 4; rid[11::101] = 255
    exp, ekeys = eref.recover_many(sigs, rid, msgs)
    assert 0 < exp.sum() < n and len(set(rid.tolist())) == 6
    got, keys = engine.ecdsa_recover_batch(sigs, rid, msgs)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]
    assert np.array_equal(keys, ekeys)
    assert not keys[exp == 0].any()
    # device form
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0"); d_keys = torch.full((n, 64), 7, dtype=torch.uint8, device="cuda:0")
    d_sig, d_rid, d_msg = _dev(sigs), _dev(rid), _dev(msgs)
    engine.ecdsa_recover_batch_dev(d_res, d_keys, d_sig, d_rid, d_msg)
    engine.sync()
    assert np.array_equal(d_res.cpu().numpy(), exp) and np.array_equal(d_keys.cpu().numpy(), ekeys)
    # recovered keys fed back as pk_format 1
    back = engine.ecdsa_verify_batch(sigs, msgs, keys, sig_format=0, pk_format=1)
    low_s = np.array([sigs[i, 32] < 0x7F for i in range(n)])          # (a flipped top bit of s makes it high: recovery takes it, verification does not)
    assert np.array_equal(back[low_s], exp[low_s])
    # the edge list
    cases = recover_cases(eref, np.random.default_rng(15))
    S = np.frombuffer(b"".join(c[1] for c in cases), np.uint8).reshape(-1, 64); R = np.array([c[2] for c in cases], np.uint8)
    M = np.frombuffer(b"".join(c[3] for c in cases), np.uint8).reshape(-1, 32)
    got, keys = engine.ecdsa_recover_batch(S, R, M)
    assert [int(x) for x in got] == [c[4] for c in cases], [c[0] for c, g in zip(cases, got) if g != c[4]]
    assert keys.tobytes() == b"".join(c[5] for c in cases)


def test_group(engine, eref, batch):
    """two engines behind one handle (both on device 0 when the box has one GPU): equal to the single-engine result, DER included"""
    import torch
    from secp256k1_zkp_amd import Group
    g = Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0])
    try:
        n = 1001
        sigs = eref.sigs_as(batch["sigobj"][:n], 0); pks = eref.pks_as(batch["pkobj"][:n], 2); msgs = batch["msgs"][:n].copy()
        msgs[::9, 5] ^= 8
        one = engine.ecdsa_verify_batch(sigs, msgs, pks, pk_format=2)
        assert 0 < one.sum() < n and np.array_equal(one, eref.verify_many(sigs, 0, msgs, pks, 2))
        assert np.array_equal(g.ecdsa_verify_batch(sigs, msgs, pks, pk_format=2), one)
        ders = eref.sigs_as(batch["sigobj"][:n], 2)
        assert np.array_equal(g.ecdsa_verify_batch(ders, msgs, pks, sig_format=2, pk_format=2), one)
        for k in (1, 2, 3):
            assert np.array_equal(g.ecdsa_verify_batch(ders[:k], msgs[:k], pks[:k], sig_format=2, pk_format=2), one[:k])
    finally:
        g.close()


def test_single_item_forms(engine, eref, batch, rec):
    """secp256k1_ecdsa_verify_amd / secp256k1_ecdsa_recover_amd on the reference's own objects; NULL arguments: 0 with the argument status"""
    L = engine._lib
    for i in range(4):
        so, m, po = batch["sigobj"][i].tobytes(), batch["msgs"][i].tobytes(), batch["pkobj"][i].tobytes()
        assert L.secp256k1_ecdsa_verify_amd(None, so, m, po) == 1 == eref.verify_obj(so, m, po)
        m2 = bytes([m[0] ^ 1]) + m[1:]
        assert L.secp256k1_ecdsa_verify_amd(None, so, m2, po) == 0 == eref.verify_obj(so, m2, po)
        assert L.s2k_last_status() == 0
    msgs, sigs, recids, pkobj = rec
    for i in range(4):
        ro = eref.recoverable_obj(sigs[i].tobytes(), int(recids[i]))
        out = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_ecdsa_recover_amd(None, out, ro, msgs[i].tobytes()) == 1 and out.raw == pkobj[i].tobytes()
        other = eref.recoverable_obj(sigs[i].tobytes(), int(recids[i]) ^ 2)
        v, pk = eref.recover(sigs[i].tobytes(), int(recids[i]) ^ 2, msgs[i].tobytes())
        assert L.secp256k1_ecdsa_recover_amd(None, out, other, msgs[i].tobytes()) == v and out.raw == pk and L.s2k_last_status() == 0
    so, m, po = batch["sigobj"][0].tobytes(), batch["msgs"][0].tobytes(), batch["pkobj"][0].tobytes()
    out = ctypes.create_string_buffer(64)
    for args in ((None, None, m, po), (None, so, None, po), (None, so, m, None)):
        assert L.secp256k1_ecdsa_verify_amd(*args) == 0 and L.s2k_last_status() == 2
    ro = eref.recoverable_obj(sigs[0].tobytes(), int(recids[0]))
    for args in ((None, None, ro, m), (None, out, None, m), (None, out, ro, None)):
        assert L.secp256k1_ecdsa_recover_amd(*args) == 0 and L.s2k_last_status() == 2
    # batch calls: NULL arrays fail the call with the argument status, n == 0 succeeds
    h = engine._h
    assert L.secp256k1_ecdsa_verify_batch(h, None, None, None, 0, None, None, 0, 4) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ecdsa_recover_batch(h, None, None, None, None, None, 4) == 0 and L.s2k_last_status() == 2
    assert L.secp256k1_ecdsa_verify_batch(h, None, None, None, 0, None, None, 0, 0) == 1
    res = np.zeros(1, np.int32)
    assert L.secp256k1_ecdsa_verify_batch(h, res.ctypes.data, so, None, 5, m, po, 1, 1) == 0 and L.s2k_last_status() == 2      # unknown sig_format
