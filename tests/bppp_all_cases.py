"""The batches of the one-verdict BP++ norm-argument verifier's tests, shared by the CPU tier (the host emulation) and the GPU tier (the
engine).  A batch is the tuple of the batch API, (proofs, trs, rhos, gens, g_len, cvs, commits); a `call` is
    call(batch, locate) -> (verdict, results or None, seed32)
and every expected verdict is the reference's own (tests/refapi.py: bppp_verify_many)."""
import json
import os

import numpy as np

from tests import bppp_all_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 8), (8, 2), (4, 4), (64, 8), (256, 1)]        # (g_len, h_len) the reference proves and accepts
SHA256_INIT_STATE = (np.array([0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19], "<u4").tobytes() + bytes(72))
_cache = {}


def n_rounds(g_len, h_len):
    return max(int(g_len).bit_length(), int(h_len).bit_length()) - 1


def random_batch(shape, n, seed=0):
    """random bytes of the right sizes (for the hashes and the scalars; no proof among them verifies)"""
    g_len, h_len = shape
    rng = np.random.default_rng(100000 * g_len + 1000 * h_len + n + seed)
    r = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    return r(n, 65 * n_rounds(g_len, h_len) + 64), r(n, 104), r(n, 32), r(g_len + h_len, 33), g_len, r(n, h_len, 32), r(n, 33)


def valid_batch(ref, shape, n):
    """n proofs of the reference's prover (made once per shape and never changed: callers copy)"""
    have = _cache.get(shape)
    if have is None or have[2].shape[0] < n:
        have = _cache[shape] = ref.make_bppp(max(n, 20), np.random.default_rng(7000 + 300 * shape[0] + shape[1]), *shape)
    p, t, r, g, gl, c, m = have
    return p[:n], t[:n], r[:n], g, gl, c[:n], m[:n]


def copy(batch):
    return tuple(x.copy() if isinstance(x, np.ndarray) else x for x in batch)


def _set(a, idx, v):
    a[idx] = v


_NB = np.frombuffer(R.N.to_bytes(32, "big"), np.uint8)
# (name, f(batch, i)): needs n_rounds >= 1
CORRUPTIONS = [
    ("an X byte", lambda b, i: _set(b[0], (i, 1 + 5), b[0][i, 1 + 5] ^ 1)),
    ("an R byte", lambda b, i: _set(b[0], (i, 33 + 7), b[0][i, 33 + 7] ^ 0x10)),
    ("the sign byte of a round", lambda b, i: _set(b[0], (i, 65 * (n_rounds(b[4], b[5].shape[1]) - 1)), b[0][i, 65 * (n_rounds(b[4], b[5].shape[1]) - 1)] ^ 1)),
    ("n", lambda b, i: _set(b[0], (i, b[0].shape[1] - 33), b[0][i, b[0].shape[1] - 33] ^ 1)),
    ("l", lambda b, i: _set(b[0], (i, b[0].shape[1] - 1), b[0][i, b[0].shape[1] - 1] ^ 1)),
    ("n = the group order", lambda b, i: _set(b[0], (i, slice(b[0].shape[1] - 64, b[0].shape[1] - 32)), _NB)),
    ("rho", lambda b, i: _set(b[2], (i, 31), b[2][i, 31] ^ 1)),
    ("rho = 0", lambda b, i: _set(b[2], i, 0)),
    ("a c_vec entry", lambda b, i: _set(b[5], (i, 0, 31), b[5][i, 0, 31] ^ 1)),
    ("the commitment", lambda b, i: _set(b[6], (i, 5), b[6][i, 5] ^ 1)),
    ("a transcript state word", lambda b, i: _set(b[1], (i, 3), b[1][i, 3] ^ 1)),
]


def positions(n):
    return sorted({0, n // 2, n - 1})


def check_against_reference(call, ref, batch, locate=True):
    """verdict == AND of the reference's verdicts; results == them element-wise; returns the verdict"""
    exp = ref.bppp_verify_many(*batch)
    v, res, _ = call(batch, locate)
    assert v == int(exp.all()), (v, exp.tolist())
    if locate:
        assert res.tolist() == exp.tolist()
    return v


def check_valid(call, ref, shape, n):
    batch = valid_batch(ref, shape, n)
    v, res, seed = call(batch, True)
    assert v == 1 and res.tolist() == [1] * n, (shape, n)
    assert seed == R.seed(*batch)
    assert call(batch, False)[0] == 1


def check_corrupted(call, ref, shape, n, where=None, kinds=None):
    for name, f in CORRUPTIONS:
        if kinds is not None and name not in kinds:
            continue
        for i in (positions(n) if where is None else where):
            b = copy(valid_batch(ref, shape, n))
            f(b, i)
            exp = ref.bppp_verify_many(*b)
            assert exp[i] == 0 and exp.sum() == n - 1, (name, i)
            assert check_against_reference(call, ref, b) == 0, (name, i)


def vectors():
    g = json.load(open(os.path.join(HERE, "golden", "bppp_verify_vectors.json")))
    gens = np.frombuffer(bytes.fromhex(g["gens"]), np.uint8).reshape(-1, 33)
    tr = np.frombuffer(SHA256_INIT_STATE, np.uint8)
    out = []
    for v in g["vectors"]:
        g_len, h_len = v["n_vec_len"], len(v["c_vec"])
        proof = np.frombuffer(bytes.fromhex(v["proof"]), np.uint8)
        cv = np.frombuffer(b"".join(bytes.fromhex(c) for c in v["c_vec"]), np.uint8).reshape(1, h_len, 32)
        batch = (proof.reshape(1, -1).copy(), tr.reshape(1, 104).copy(), np.frombuffer(bytes.fromhex(v["rho"]), np.uint8).reshape(1, 32).copy(),
                 gens[:g_len + h_len].copy(), g_len, cv.copy(), np.frombuffer(bytes.fromhex(v["commit33"]), np.uint8).reshape(1, 33).copy())
        out.append((v["index"], batch, v["result"]))
    return out


def prove_over(ref, gens, g_len, h_len, n, rng):
    """n proofs of the reference's prover over a GIVEN generator set (the flow of refapi.Ref.make_bppp, which fixes its own set)"""
    import ctypes
    gens = np.ascontiguousarray(gens, np.uint8); ng = ctypes.c_size_t(g_len + h_len)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    sc = lambda k: (rng.integers(0, 256, (k, 32), dtype=np.uint8) & np.array([0x7F] + [0xFF] * 31, np.uint8))
    plen = 65 * n_rounds(g_len, h_len) + 64
    proofs = np.zeros((n, plen), np.uint8); trs = np.zeros((n, 104), np.uint8); rhos = sc(n)
    cvs = np.zeros((n, h_len, 32), np.uint8); commits = np.zeros((n, 33), np.uint8)
    for i in range(n):
        nv, lv, cv = sc(g_len), sc(h_len), sc(h_len)
        mu = np.zeros(32, np.uint8); cm = np.zeros(33, np.uint8); tr = np.zeros(104, np.uint8); pr = np.zeros(plen, np.uint8); pl = ctypes.c_size_t(plen)
        ref.lib.ref_scalar_mul(p(mu), p(rhos[i]), p(rhos[i]))
        assert ref.lib.ref_bppp_commit(p(cm), p(gens), ng, p(nv), ctypes.c_size_t(g_len), p(lv), p(cv), ctypes.c_size_t(h_len), p(mu)) == 1
        ref.lib.ref_bppp_transcript_init(p(tr), p(rhos[i]), p(gens), ng, ctypes.c_size_t(g_len), p(cv), ctypes.c_size_t(h_len), p(cm))
        assert ref.lib.ref_bppp_norm_prove(p(pr), ctypes.byref(pl), p(tr), p(rhos[i]), p(gens), ng, p(nv), ctypes.c_size_t(g_len), p(lv), p(cv), ctypes.c_size_t(h_len)) == 1
        assert pl.value == plen
        proofs[i] = pr; trs[i] = tr; cvs[i] = cv; commits[i] = cm
    return proofs, trs, rhos, gens, g_len, cvs, commits


def check_vectors(call, ref):
    """the 13 vectors alone, and embedded among five valid proofs over the vectors' own generators wherever the vector's shape is one the
    reference accepts (ten of them; the others are a 63-byte proof, g_len 0 and a c_vec the proof length does not match)"""
    vec = vectors()
    assert len(vec) == 13
    embedded = 0
    for index, batch, result in vec:
        v, res, _ = call(batch, True)
        assert v == result and res.tolist() == [result], index
        g_len, h_len = batch[4], batch[5].shape[1]
        if g_len == 0 or batch[0].shape[1] != 65 * n_rounds(g_len, h_len) + 64:
            assert result == 0
            continue
        key = ("vectors", g_len, h_len)
        if key not in _cache:
            _cache[key] = prove_over(ref, batch[3], g_len, h_len, 5, np.random.default_rng(50 + 10 * g_len + h_len))
        good = _cache[key]
        for at in (0, 2, 5):
            b = tuple(np.concatenate([x[:at], y, x[at:]]) if k not in (3, 4) else x for k, (x, y) in enumerate(zip(good, batch)))
            exp = ref.bppp_verify_many(*b)
            assert exp[at] == result and exp.sum() == 5 + result, index
            assert check_against_reference(call, ref, b) == result, (index, at)
        embedded += 1
    assert embedded >= 10, embedded


def tweak_commit(tw, commit33, t):
    """commit + t G through the reference's secp256k1_ec_pubkey_tweak_add"""
    obj = tw.ec_parse(commit33.tobytes())
    assert obj is not None
    out = tw.ec_tweak_add(obj, (t % R.N).to_bytes(32, "big"))
    assert out is not None
    return np.frombuffer(tw.ec_serialize(out), np.uint8)


def check_cancellation(call, ref, tw, shape, n):
    """commit_j + t G and commit_k - t G: with equal coefficients the two defects would cancel"""
    t = 0x1234567
    for j, k in {(0, n - 1), (0, 1), (1, n - 1)}:
        if j == k or k >= n:
            continue
        b = copy(valid_batch(ref, shape, n))
        b[6][j] = tweak_commit(tw, b[6][j], t); b[6][k] = tweak_commit(tw, b[6][k], -t)
        exp = ref.bppp_verify_many(*b)
        assert exp[j] == 0 and exp[k] == 0 and exp.sum() == n - 2
        assert check_against_reference(call, ref, b) == 0, (j, k)


def check_coincident(call, ref, shape=(4, 4)):
    one = valid_batch(ref, shape, 1)
    b = tuple(np.concatenate([x] * 20) if k not in (3, 4) else x for k, x in enumerate(one))
    v, res, _ = call(b, True)
    assert v == 1 and res.tolist() == [1] * 20
    b = copy(b); b[0][13, 40] ^= 2
    assert check_against_reference(call, ref, b) == 0


def check_infinity_encodings(call, ref):
    """an all-zero commitment (vector 9: accepted), X and R encoded as infinity (vector 10: accepted) and a zero x under a set sign bit, which
    is no encoding at all (vector 11), alone: the sum must take pt_inf"""
    by = {index: (batch, result) for index, batch, result in vectors()}
    assert not by[9][0][6].any() and by[9][1] == 1
    assert by[10][1] == 1 and by[10][0][0][0, 0] == 0 and by[11][1] == 0 and by[11][0][0][0, 0] == 1
    for index in (9, 10, 11):
        batch, result = by[index]
        if index != 9:
            assert not batch[0][0, 1:65].any()
        assert ref.bppp_verify_many(*batch)[0] == result
        assert call(batch, False)[0] == result, index
    # and an all-zero commitment in a batch of valid proofs: refused, as the reference refuses that proof
    b = copy(valid_batch(ref, (4, 4), 5)); b[6][2] = 0
    assert check_against_reference(call, ref, b) == 0
    b = copy(valid_batch(ref, (4, 4), 5)); b[0][4, 0] = 0; b[0][4, 1:33] = 0          # X_0 of the last proof: infinity
    assert check_against_reference(call, ref, b) == 0


def check_empty(call):
    z = lambda *s: np.zeros(s, np.uint8)
    v, res, seed = call((z(0, 194), z(0, 104), z(0, 32), z(8, 33), 4, z(0, 4, 32), z(0, 33)), True)
    assert v == 1 and len(res) == 0 and seed == bytes(32)
