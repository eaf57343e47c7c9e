"""Plain-Python restatement of the one-verdict BIP-340 batch verifier (secp256k1_zkp_amd/csrc/schnorr_all.h): the coefficient derivation
with hashlib, the per-item BIP-340 check with integers, and a small signer that takes the nonce as an argument, so that tests can make
signatures the reference's signer never makes (nonce equal to the secret key, one nonce for two messages, one key for a whole batch).
Nothing here is constant time and nothing here is fast: it is the specification the emulator and the device are pinned against."""
import hashlib

import numpy as np

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
FANIN = 16


# ---- the derivation -------------------------------------------------------------------------------------------------------------------
def T(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


def key_x32(pk, pk_format):
    """the 32 bytes of a key as the item digest hashes them: the serialisation itself, or the object's x (little-endian in memory) reversed"""
    pk = bytes(pk)
    return pk[:32] if pk_format == 0 else pk[:32][::-1]


def item_digest(sig, pk, msg, pk_format=0):
    return T("S2K/schnorr_all/item", bytes(sig) + key_x32(pk, pk_format) + bytes(msg))


def level_plan(n):
    counts = []
    while n:
        counts.append(n)
        if n == 1:
            break
        n = (n + FANIN - 1) // FANIN
    return counts


def root(digests):
    level = list(digests)
    while len(level) > 1:
        level = [T("S2K/schnorr_all/node", b"".join(level[j:j + FANIN])) for j in range(0, len(level), FANIN)]
    return level[0]


def _rows(a, width, n):
    a = np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, np.uint8)
    return [a.reshape(-1)[width * i:width * (i + 1)].tobytes() for i in range(n)]


def seed(sigs, msgs, pks, msglen=32, pk_format=0):
    """the seed of a batch given as flat byte arrays (n*64, n*msglen, n*32 or n*64); n = 0: 32 zero bytes"""
    n = np.asarray(sigs).size // 64 if not isinstance(sigs, (bytes, bytearray)) else len(sigs) // 64
    if n == 0:
        return bytes(32)
    s, m, k = _rows(sigs, 64, n), _rows(msgs, msglen, n), _rows(pks, 64 if pk_format else 32, n)
    r = root([item_digest(s[i], k[i], m[i], pk_format) for i in range(n)])
    return T("S2K/schnorr_all/seed", n.to_bytes(8, "little") + msglen.to_bytes(8, "little") + r)


def coefficient(seed32, i):
    if i == 0:
        return 1
    a = int.from_bytes(T("S2K/schnorr_all/rand", seed32 + i.to_bytes(8, "little"))[:16], "big")
    return a or 1


def coefficients(seed32, n):
    return [coefficient(seed32, i) for i in range(n)]


# ---- the curve, with integers ---------------------------------------------------------------------------------------------------------
def _jdbl(p):
    x, y, z = p
    if not y:
        return (0, 0, 0)
    s = 4 * x * y * y % P; m = 3 * x * x % P
    nx = (m * m - 2 * s) % P
    return (nx, (m * (s - nx) - 8 * y * y * y * y) % P, 2 * y * z % P)


def _jadd(p, q):
    if not p[2]:
        return q
    if not q[2]:
        return p
    x1, y1, z1 = p; x2, y2, z2 = q
    z1z, z2z = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * z2z % P, x2 * z1z % P
    s1, s2 = y1 * z2z * z2 % P, y2 * z1z * z1 % P
    if u1 == u2:
        return _jdbl(p) if s1 == s2 else (0, 0, 0)
    h, r = (u2 - u1) % P, (s2 - s1) % P
    h2 = h * h % P; h3 = h2 * h % P; v = u1 * h2 % P
    nx = (r * r - h3 - 2 * v) % P
    return (nx, (r * (v - nx) - s1 * h3) % P, h * z1 * z2 % P)


def _affine(p):
    if not p[2]:
        return None
    zi = pow(p[2], P - 2, P); zi2 = zi * zi % P
    return (p[0] * zi2 % P, p[1] * zi2 * zi % P)


def mul(k, pt=G):
    """k * pt as an affine pair, None for infinity"""
    k %= N
    acc, base = (0, 0, 0), (pt[0], pt[1], 1)
    while k:
        if k & 1:
            acc = _jadd(acc, base)
        base = _jdbl(base); k >>= 1
    return _affine(acc)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return _affine(_jadd((a[0], a[1], 1), (b[0], b[1], 1)))


def lift_x(x):
    """the point with this x and even y, None if x >= p or not on the curve"""
    if x >= P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return (x, y if y % 2 == 0 else P - y)


def challenge(r32, px32, msg):
    return int.from_bytes(T("BIP0340/challenge", bytes(r32) + bytes(px32) + bytes(msg)), "big") % N


def verify(sig, msg, pk32):
    """secp256k1_schnorrsig_verify on a serialised x-only key"""
    sig, msg, pk32 = bytes(sig), bytes(msg), bytes(pk32)
    Pk = lift_x(int.from_bytes(pk32, "big"))
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if Pk is None or r >= P or s >= N:
        return 0
    e = challenge(sig[:32], pk32, msg)
    R = add(mul(s), mul(N - e, Pk))
    return int(R is not None and R[1] % 2 == 0 and R[0] == r)


def verify_many(sigs, msgs, pks32, msglen=32):
    n = np.asarray(sigs).size // 64
    s, m, k = _rows(sigs, 64, n), _rows(msgs, msglen, n), _rows(pks32, 32, n)
    return np.array([verify(s[i], m[i], k[i]) for i in range(n)], np.int32)


def verify_all(sigs, msgs, pks32, msglen=32):
    """the batch equation itself, with the derived coefficients (format 0): what the engine's call computes"""
    n = np.asarray(sigs).size // 64
    if n == 0:
        return 1
    s, m, k = _rows(sigs, 64, n), _rows(msgs, msglen, n), _rows(pks32, 32, n)
    a = coefficients(seed(sigs, msgs, pks32, msglen, 0), n)
    acc, g = None, 0
    for i in range(n):
        r, si = int.from_bytes(s[i][:32], "big"), int.from_bytes(s[i][32:], "big")
        R, Pk = lift_x(r), lift_x(int.from_bytes(k[i], "big"))
        if R is None or Pk is None or si >= N:
            return 0
        e = challenge(s[i][:32], k[i], m[i])
        acc = add(acc, add(mul(a[i], R), mul(a[i] * e, Pk)))
        g = (g + a[i] * si) % N
    return int(add(acc, mul(N - g)) is None)


def pubkey(d):
    """(the secret key as BIP-340 uses it, the serialised x-only key)"""
    Q = mul(d)
    return (d if Q[1] % 2 == 0 else N - d), Q[0].to_bytes(32, "big")


def sign(d, msg, k):
    """a BIP-340 signature of msg under secret key d with the nonce k, whatever k is (1 <= k < n)"""
    d, px = pubkey(d)
    R = mul(k)
    if R[1] % 2:
        k = N - k
    r32 = R[0].to_bytes(32, "big")
    e = challenge(r32, px, msg)
    return r32 + ((k + e * d) % N).to_bytes(32, "big"), px


def objects(pks32):
    """serialised x-only keys -> 64-byte secp256k1_xonly_pubkey objects as the reference holds them on a little-endian host (x | y, each
    least significant byte first); every key must be valid"""
    out = []
    for pk in _rows(pks32, 32, np.asarray(pks32).size // 32):
        x, y = lift_x(int.from_bytes(pk, "big"))
        out.append(x.to_bytes(32, "little") + y.to_bytes(32, "little"))
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 64).copy()


def pack(items):
    """[(sig, msg, pk32)] -> flat arrays"""
    f = lambda j, w: np.frombuffer(b"".join(bytes(t[j]) for t in items), np.uint8).reshape(len(items), w).copy() if w else np.zeros((len(items), 0), np.uint8)   # noqa: E731
    return f(0, 64), f(1, len(items[0][1])), f(2, 32)


# ---- the batches the reference's signer never makes -------------------------------------------------------------------------------------
def coincident_batches(count=20):
    """name -> [(sig, msg, pk32)] of `count` valid signatures whose points coincide"""
    msgs = [hashlib.sha256(b"schnorr_all %d" % i).digest() for i in range(count)]
    out = {}
    items = []                                        # the nonce IS the secret key: R_i == P_i
    for i in range(count):
        d = int.from_bytes(hashlib.sha256(b"key %d" % i).digest(), "big") % N
        sig, px = sign(d, msgs[i], pubkey(d)[0])
        items.append((sig, msgs[i], px))
    out["nonce_is_key"] = items
    items = []                                        # one nonce for two messages: R_i == R_j (different keys)
    for i in range(count):
        d = int.from_bytes(hashlib.sha256(b"key %d" % i).digest(), "big") % N
        k = int.from_bytes(hashlib.sha256(b"nonce %d" % (i // 2)).digest(), "big") % N
        sig, px = sign(d, msgs[i], k)
        items.append((sig, msgs[i], px))
    out["shared_nonce"] = items
    items = []                                        # one key for the whole batch
    d = int.from_bytes(hashlib.sha256(b"the key").digest(), "big") % N
    for i in range(count):
        k = int.from_bytes(hashlib.sha256(b"nonce' %d" % i).digest(), "big") % N
        sig, px = sign(d, msgs[i], k)
        items.append((sig, msgs[i], px))
    out["one_key"] = items
    out["repeated"] = [items[0]] * count             # one valid signature, `count` times
    return out
