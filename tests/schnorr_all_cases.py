"""The batches of the one-verdict BIP-340 verifier's tests, shared by the CPU tier (the host emulation) and the GPU tier (the engine).
A `call` is  call(sigs, msgs, pks, msglen, pk_format, locate) -> (verdict, results or None, seed32)  over numpy byte arrays."""
import json
import os

import numpy as np

from tests import schnorr_all_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def random_batch(n, msglen, seed=0):
    rng = np.random.default_rng(1000 * n + msglen + seed)
    return rng.integers(0, 256, (n, 64), dtype=np.uint8), rng.integers(0, 256, (n, msglen), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)


def valid_batch(ref, n):
    """n signatures of the reference's signer (made once per size and never changed: callers copy)"""
    if n not in _cache:
        _cache[n] = ref.make_schnorr(n, np.random.default_rng(340 + n))
    return _cache[n]


def vectors():
    """msglen -> (passing [(sig, msg, pk)], failing [(sig, msg, pk)]) of tests/golden/bip340_vectors.json"""
    out = {}
    for v in json.load(open(os.path.join(HERE, "golden", "bip340_vectors.json")))["vectors"]:
        t = (bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["pk"]))
        out.setdefault(len(t[1]), ([], []))[0 if v["result"] else 1].append(t)
    return out


def _flip(a, i, byte, bit=0):
    a[i, byte] ^= 1 << bit


CORRUPTIONS = [
    ("a bit of s", lambda s, m, k, i: _flip(s, i, 63)),
    ("a bit of r", lambda s, m, k, i: _flip(s, i, 5, 3)),
    ("a bit of the message", lambda s, m, k, i: _flip(m, i, 17, 7)),
    ("a bit of the key", lambda s, m, k, i: _flip(k, i, 31, 1)),
    ("s = ff..", lambda s, m, k, i: s.__setitem__((i, slice(32, 64)), 0xFF)),
    ("r = ff..", lambda s, m, k, i: s.__setitem__((i, slice(0, 32)), 0xFF)),
]


def positions(n):
    return sorted({0, n // 2, n - 1})


def check_vectors(call):
    vec = vectors()
    assert sorted(vec) == [0, 1, 17, 32, 100] and len(vec[32][0]) == 5 and len(vec[32][1]) == 10
    for msglen, (good, bad) in vec.items():
        s, m, k = R.pack(good)
        v, res, _ = call(s, m, k, msglen, 0, True)
        assert v == 1 and res.tolist() == [1] * len(good), msglen
        assert call(s, m, R.objects(k), msglen, 1, False)[0] == 1, msglen
        for b in bad:
            for at in (0, len(good)):
                items = good[:at] + [b] + good[at:]
                s, m, k = R.pack(items)
                v, res, _ = call(s, m, k, msglen, 0, True)
                assert v == 0 and res.tolist() == [int(t is not b) for t in items], (msglen, b[0].hex())


def check_valid(call, ref, n):
    s, m, k = valid_batch(ref, n)
    seeds = []
    for f, keys in ((0, k), (1, ref.xonly_objects(k))):
        v, res, seed = call(s, m, keys, 32, f, True)
        assert v == 1 and res.tolist() == [1] * n, (n, f)
        seeds.append(seed)
    assert seeds[0] == seeds[1] == R.seed(s, m, k, 32, 0)


def check_corrupted(call, ref, n, where=None):
    s0, m0, k0 = valid_batch(ref, n)
    for name, spoil in CORRUPTIONS:
        for i in (positions(n) if where is None else where):
            s, m, k = s0.copy(), m0.copy(), k0.copy()
            spoil(s, m, k, i)
            v, res, _ = call(s, m, k, 32, 0, True)
            want = ref.schnorr_verify_many(s, m, k)
            assert want[i] == 0 and int(want.sum()) == n - 1
            assert v == 0 and res.tolist() == want.tolist(), (n, name, i)


def _s_add(s, i, d):
    v = (int.from_bytes(s[i, 32:].tobytes(), "big") + d) % R.N
    s[i, 32:] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)


def check_cancellation(call, ref, n):
    """s_j + 1 and s_k - 1: the plain sum of the s_i is unchanged, so with equal coefficients the batch equation would still hold"""
    s0, m, k = valid_batch(ref, n)
    assert call(s0, m, k, 32, 0, False)[0] == 1
    for j, q in sorted({(0, 1), (0, n - 1), (n - 2, n - 1)}):
        s = s0.copy(); _s_add(s, j, 1); _s_add(s, q, -1)
        v, res, _ = call(s, m, k, 32, 0, True)
        assert v == 0 and res.tolist() == [int(i not in (j, q)) for i in range(n)], (n, j, q)
        s = s0.copy(); s[[j, q], 32:] = s[[q, j], 32:]
        assert call(s, m, k, 32, 0, False)[0] == 0, (n, j, q, "exchanged")


def check_coincident(call):
    for name, items in R.coincident_batches(20).items():
        s, m, k = R.pack(items)
        assert R.verify_many(s, m, k).tolist() == [1] * 20, name
        for f, keys in ((0, k), (1, R.objects(k))):
            assert call(s, m, keys, 32, f, False)[0] == 1, (name, f)
        s2 = s.copy(); _flip(s2, 7, 40)
        v, res, _ = call(s2, m, k, 32, 0, True)
        assert v == 0 and res.tolist() == [int(i != 7) for i in range(20)], name


def check_empty(call):
    e = np.zeros((0, 64), np.uint8)
    for msglen in (0, 32):
        v, res, seed = call(e, np.zeros((0, msglen), np.uint8), np.zeros((0, 32), np.uint8), msglen, 0, True)
        assert v == 1 and len(res) == 0 and seed == bytes(32)
