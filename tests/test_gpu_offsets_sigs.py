"""GPU: where BIP-340 and ECDSA verification place an item in a batch (csrc/engine_core.hip: secp256k1_schnorrsig_verify_batch_group and
the launch loop of secp256k1_schnorrsig_verify_batch_dev; csrc/engine_ecdsa.hip; csrc/engine_lanes.h: lanes_run).  Group shares that
start at lo > 0 with 64-byte key objects and messages of other lengths than 32; launches that start at i0 > 0 with keys of 64 and 65
bytes.  The verdicts are the reference's (oracle/_ref).  tests/batch_edges.py asserts before every call that the batch could show a
wrong stride or a dropped offset."""
import ctypes

import numpy as np
import pytest

from tests import batch_edges as E
from tests import schnorr_all_ref as R
from tests.test_gpu_ecdsa import PK_BYTES, _verify_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groups():
    """three engines on device 0 (shares start at n/3 and 2n/3, and are empty below three items), and two engines on two devices where
    there are two"""
    import torch
    from secp256k1_zkp_amd import Group
    made = []
    try:
        made.append(Group([0, 0, 0]))
        made.append(Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0]))
        yield made
    finally:
        for g in made:
            g.close()


@pytest.fixture(scope="module")
def bip340_keys():
    """599 key pairs and 599 nonces for the Python signer (tests/schnorr_all_ref.py: the reference's own signs 32-byte messages only):
    d0 + i and k0 + i, every point one addition of G away from the last; -> [(d, px32, k, r32)] with d and k as BIP-340 uses them"""
    d, k = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F90A1B2C3D4E5F60718293A4B5C6D7E8, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F1
    Q, Rp = R.mul(d), R.mul(k)
    out = []
    for i in range(599):
        out.append((d + i if Q[1] % 2 == 0 else R.N - d - i, Q[0].to_bytes(32, "big"), k + i if Rp[1] % 2 == 0 else R.N - k - i, Rp[0].to_bytes(32, "big")))
        Q, Rp = R.add(Q, R.G), R.add(Rp, R.G)
    return out


def _bip340_batch(keys, n, msglen, seed):
    """n signatures of msglen-byte messages, one in nine with a flipped bit of s (and every thirteenth message with one, where there are
    messages); -> (sigs, msgs, serialised keys, key objects)"""
    rng = np.random.default_rng(seed)
    msgs = rng.integers(0, 256, (n, msglen), dtype=np.uint8)
    sigs = np.zeros((n, 64), np.uint8)
    for i, (d, px, k, r32) in enumerate(keys[:n]):
        sigs[i] = np.frombuffer(r32 + ((k + R.challenge(r32, px, msgs[i].tobytes()) * d) % R.N).to_bytes(32, "big"), np.uint8)
    sigs[8::9, 40] ^= 1
    if msglen:
        msgs[12::13, msglen // 2] ^= 0x10
    pks = np.frombuffer(b"".join(x[1] for x in keys[:n]), np.uint8).reshape(n, 32).copy()
    return sigs, msgs, pks, R.objects(pks)


def test_group_shares_bip340_key_objects_and_message_lengths(groups, bip340_keys, ref):
    """secp256k1_schnorrsig_verify_batch_group with 64-byte key objects and messages of 0, 17, 32 and 65 bytes: every share but the first
    starts at lo > 0, where the form adds 64 * lo, msglen * lo and pkb * lo to the caller's arrays (and must hand on a NULL message
    array as it is).  599 items on three engines (starts 199 and 399) and on two (299); 1 .. 5 leave engines idle.  Every item has its
    own key, nonce and message; the verdicts are the reference's, which agrees that the Python signer's signatures are valid."""
    L = groups[0]._lib
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for msglen in (17, 0, 32, 65):
        for n in (1, 2, 3, 4, 5, 65, 257, 599) if msglen == 17 else (599, 4):
            sigs, msgs, pks, objs = _bip340_batch(bip340_keys, n, msglen, 1210 + msglen)
            exp = ref.schnorr_verify_many(sigs, msgs, pks, msglen=msglen)
            bad = np.zeros(n, bool); bad[8::9] = True
            if msglen:
                bad[12::13] = True
            assert np.array_equal(exp, (~bad).astype(np.int32)), (msglen, n)
            for g in groups:
                arrays = dict(sigs=sigs, pks=objs, msgs=msgs) if msglen else dict(sigs=sigs, pks=objs)
                E.check((msglen, n, len(g)), E.share_starts(n, len(g)), arrays, exp, both=n >= 65)
                if msglen:
                    got = g.schnorrsig_verify_batch(sigs, msgs, objs, msglen=msglen, pk_format=1)
                else:
                    got = np.full(n, 7, np.int32)
                    assert L.secp256k1_schnorrsig_verify_batch_group(g._h, vp(got), vp(sigs), None, 0, vp(objs), 1, n) == 1
                assert np.array_equal(got, exp), (msglen, n, len(g), np.flatnonzero(got != exp)[:8])
    # a NULL array through the `_group` form: 0 with the argument status, and nothing marked valid
    res = np.full(n, 7, np.int32)
    for k in (0, 1, 2, 4):
        a = [vp(res), vp(sigs), vp(msgs), 65, vp(objs), 1, n]; a[k] = None
        assert L.secp256k1_schnorrsig_verify_batch_group(groups[0]._h, *a) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), k


def test_sub_range_launches_bip340_key_objects(ref):
    """1500 reference-made signatures, 100 of them corrupted, with 64-byte key objects on an engine whose launches take 512 lanes:
    launch i0 reads pubkeys + 64 * i0 (every item has its own key)"""
    from secp256k1_zkp_amd import Engine
    rng = np.random.default_rng(1211)
    n = 1500
    sigs, msgs, pks = ref.make_schnorr(n, rng)
    sigs[rng.choice(n, 100, replace=False), 40] ^= 1
    exp = ref.schnorr_verify_many(sigs, msgs, pks, threads=8)
    assert exp.sum() == n - 100
    objs = R.objects(pks)
    E.check("key objects", E.launch_starts(n, 512), dict(sigs=sigs, msgs=msgs, pks=objs), exp)
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 512)
        got = eng.schnorrsig_verify_batch(sigs, msgs, objs, pk_format=1)
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_sub_range_launches_ecdsa_key_objects_and_full_keys(ref):
    """1100 reference-made signatures, one in seven corrupted, with keys of 64 and of 65 bytes, compact and DER, on an engine whose
    launches take 512 lanes: launch i0 reads pubkeys + pkb * i0 (every item is its own: no two rows agree).  Host and _dev form."""
    from secp256k1_zkp_amd import Engine
    from tests.ecdsa_ref import EcdsaRef
    eref = EcdsaRef()
    batch = eref.make(1100, np.random.default_rng(2211))
    sigs = eref.sigs_as(batch["sigobj"], 0); msgs = batch["msgs"].copy()
    sigs[::7, 40] ^= 1
    ders = [eref.sig_serialize_der(o) if o is not None else b"\x30\x00" for o in (eref.sig_parse_compact(sigs[i].tobytes()) for i in range(1100))]
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 512)
        for pf in (1, 2):
            pkf = eref.pks_as(batch["pkobj"], pf)
            assert pkf.shape == (1100, PK_BYTES[pf])
            exp = eref.verify_many(sigs, 0, msgs, pkf, pf)
            assert 0 < exp.sum() < 1100
            for n in (700, 1100):
                E.check((pf, n), E.launch_starts(n, 512), dict(sigs=sigs[:n], msgs=msgs[:n], pks=pkf[:n]), exp[:n])
                E.check((pf, n, "DER"), E.launch_starts(n, 512), dict(sigs=ders[:n], msgs=msgs[:n], pks=pkf[:n]), exp[:n])
                assert np.array_equal(eng.ecdsa_verify_batch(sigs[:n], msgs[:n], pkf[:n], pk_format=pf), exp[:n]), (pf, n)
                assert np.array_equal(eng.ecdsa_verify_batch(ders[:n], msgs[:n], pkf[:n], sig_format=2, pk_format=pf), exp[:n]), (pf, n, "DER")
                assert np.array_equal(_verify_dev(eng, sigs[:n], 0, msgs[:n], pkf[:n], pf), exp[:n]), (pf, n, "dev")
                assert np.array_equal(_verify_dev(eng, ders[:n], 2, msgs[:n], pkf[:n], pf), exp[:n]), (pf, n, "DER, dev")
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()
