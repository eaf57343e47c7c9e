"""The coefficient derivation of the one-verdict BP++ norm-argument verifier (csrc/bppp_all.h) written with hashlib, and the scalars of its
one sum recomputed with Python integers from given per-proof scalars sc[p][t].  Test-only.

Batches are numpy byte arrays: proofs (n, proof_len), trs (n, 104), rhos (n, 32), gens (n_gens, 33), cvs (n, h_len, 32), commits (n, 33)."""
import hashlib
import struct

import numpy as np

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
FANIN = 16


def T(tag, x):
    t = hashlib.sha256(tag).digest()
    return hashlib.sha256(t + t + x).digest()


MU = int.from_bytes(hashlib.sha256(b"S2K/bppp_all/scale").digest(), "big") % N


def le64(v):
    return struct.pack("<Q", v)


def level_plan(n):
    out = []
    while n:
        out.append(n)
        if n == 1:
            break
        n = (n + FANIN - 1) // FANIN
    return out


def colsum_plan(n, chunk):
    """[chunks, ceil(chunks / 16), ..., 1]: the first pass and at least one fan-in pass"""
    if n == 0:
        return []
    c = (n + chunk - 1) // chunk
    out = [c]
    while True:
        c = (c + FANIN - 1) // FANIN
        out.append(c)
        if c <= 1:
            return out


def _b(a):
    return np.ascontiguousarray(a, np.uint8).tobytes()


def gens_digest(gens, g_len):
    g = _b(gens)
    return T(b"S2K/bppp_all/gens", le64(len(g) // 33) + le64(g_len) + g)


def item_digests(proofs, trs, rhos, cvs, commits):
    n = np.asarray(rhos).size // 32
    proofs, trs, rhos, cvs, commits = (np.ascontiguousarray(x, np.uint8).reshape(n, -1) for x in (proofs, trs, rhos, cvs, commits))
    return [T(b"S2K/bppp_all/item", _b(proofs[p]) + _b(trs[p]) + _b(rhos[p]) + _b(cvs[p]) + _b(commits[p])) for p in range(n)]


def root(ds):
    while len(ds) > 1:
        ds = [T(b"S2K/bppp_all/node", b"".join(ds[j:j + FANIN])) for j in range(0, len(ds), FANIN)]
    return ds[0]


def seed(proofs, trs, rhos, gens, g_len, cvs, commits):
    n = np.asarray(rhos).size // 32
    if n == 0:
        return bytes(32)
    proof_len = np.asarray(proofs).size // n; h_len = np.asarray(cvs).size // 32 // n
    return T(b"S2K/bppp_all/seed", le64(n) + le64(proof_len) + le64(h_len) + gens_digest(gens, g_len) + root(item_digests(proofs, trs, rhos, cvs, commits)))


def coefficients(seed32, n):
    out = []
    for p in range(n):
        z = 1 if p == 0 else int.from_bytes(T(b"S2K/bppp_all/rand", seed32 + le64(p))[:16], "big")
        out.append(z or 1)
    return out


def zprime(seed32, n):
    return [MU * z % N for z in coefficients(seed32, n)]


def sums(sc, zp, n_gens):
    """sc[p][t] (ints, the order of bp_term), z'_p -> (S_t for t < n_gens, g_sc, own[p][j] = z'_p sc[p][n_gens + 1 + j])"""
    S = [sum(z * row[t] for z, row in zip(zp, sc)) % N for t in range(n_gens)]
    g = sum(z * row[n_gens] for z, row in zip(zp, sc)) % N
    own = [[z * v % N for v in row[n_gens + 1:]] for z, row in zip(zp, sc)]
    return S, g, own
