"""A Python statement of secp256k1_ecdsa_adaptor_verify over plain integers (src/modules/ecdsa_adaptor/main_impl.h:236-282, dleq_impl.h
:62-76, :131-162 of the reference), a signer for it, and the edge list the adaptor tests share.  Test-only.

The reference library the other oracles use (oracle/_ref) is built without the ecdsa_adaptor module, so this model is the oracle of
the CPU tier; what ties it to the reference is tests/golden/adaptor_vectors.json, whose verdicts the reference's own function returned
when tests/golden/make_adaptor_golden.py wrote the file.

An item is the tuple
    (name, sig162, pubkey, msg32, enckey, verdict, fmt_only)
with both keys as 33 compressed bytes and fmt_only None: keys_in_format() gives them in any of the engine's three key formats.  The one
exception is the all-zero key object (fmt_only 1, both keys 64 bytes, engine only, verdict 0: the reference calls its illegal-argument
callback there).  The signer takes the nonces as arguments: how they are derived does not matter to verification."""
import hashlib

import numpy as np

from secp256k1_zkp_amd.constants import P, N, G_XY

G = (int.from_bytes(G_XY[:32], "big"), int.from_bytes(G_XY[32:], "big"))
INF = None


# ---- the curve over plain integers ------------------------------------------------------------------------------------------------------
def pt_add(a, b):
    if a is INF:
        return b
    if b is INF:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return INF
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def pt_neg(a):
    return INF if a is INF else (a[0], (P - a[1]) % P)


def _jac_double(a):
    X, Y, Z = a
    if Y == 0:
        return (0, 1, 0)
    S = 4 * X * Y * Y % P; M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return (X3, (M * (S - X3) - 8 * pow(Y, 4, P)) % P, 2 * Y * Z % P)


def _jac_add_affine(a, b):
    X, Y, Z = a
    if Z == 0:
        return (b[0], b[1], 1)
    Z2 = Z * Z % P
    U2, S2 = b[0] * Z2 % P, b[1] * Z2 * Z % P
    H, R = (U2 - X) % P, (S2 - Y) % P
    if H == 0:
        return _jac_double(a) if R == 0 else (0, 1, 0)
    H2 = H * H % P; H3 = H2 * H % P; V = X * H2 % P
    X3 = (R * R - H3 - 2 * V) % P
    return (X3, (R * (V - X3) - Y * H3) % P, Z * H % P)


def pt_mul(k, a):
    """double-and-add in Jacobian coordinates (one inversion at the end); pt_add above is the plain affine law it is tested against"""
    k %= N
    if a is INF or k == 0:
        return INF
    r = (0, 1, 0)
    for bit in bin(k)[2:]:
        r = _jac_double(r)
        if bit == "1":
            r = _jac_add_affine(r, a)
    if r[2] == 0:
        return INF
    zi = pow(r[2], -1, P)
    return (r[0] * zi * zi % P, r[1] * zi * zi * zi % P)


def lift_x(x, odd):
    """the point with this x and this parity of y, or None"""
    if x >= P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return (x, y if (y & 1) == odd else P - y)


def parse33(b):
    """secp256k1_eckey_pubkey_parse of 33 bytes"""
    if len(b) != 33 or b[0] not in (2, 3):
        return None
    return lift_x(int.from_bytes(b[1:], "big"), b[0] & 1)


def ser33(a):
    return bytes([2 + (a[1] & 1)]) + a[0].to_bytes(32, "big")


def b32(v):
    return int(v).to_bytes(32, "big")


def tagged_midstate_input():
    t = hashlib.sha256(b"DLEQ").digest()
    return t + t


def dleq_challenge(p1, gen2, p2, r1, r2):
    """secp256k1_dleq_challenge: the tagged hash over p1 | gen2 | p2 | r1 | r2, reduced mod n"""
    h = hashlib.sha256(tagged_midstate_input() + ser33(p1) + ser33(gen2) + ser33(p2) + ser33(r1) + ser33(r2)).digest()
    return int.from_bytes(h, "big") % N


# ---- the verifier and a signer ----------------------------------------------------------------------------------------------------------
def verify(sig162, pubkey33, msg32, enckey33):
    """keys as 33 compressed bytes (what secp256k1_ec_pubkey_parse accepts of them); returns 0 or 1"""
    sig162 = bytes(sig162)
    R = parse33(sig162[0:33])
    if R is None:
        return 0
    sigr = int.from_bytes(sig162[1:33], "big") % N
    if sigr == 0:
        return 0
    Rp = parse33(sig162[33:66])
    if Rp is None:
        return 0
    sp = int.from_bytes(sig162[66:98], "big")
    if sp == 0 or sp >= N:
        return 0
    e = int.from_bytes(sig162[98:130], "big") % N
    s = int.from_bytes(sig162[130:162], "big")
    if s >= N:
        return 0
    Y = parse33(bytes(enckey33))
    if Y is None:
        return 0
    R1 = pt_add(pt_mul(s, G), pt_neg(pt_mul(e, Rp)))
    R2 = pt_add(pt_mul(s, Y), pt_neg(pt_mul(e, R)))
    if R1 is INF or R2 is INF:
        return 0
    if dleq_challenge(Rp, Y, R, R1, R2) != e:
        return 0
    X = parse33(bytes(pubkey33))
    if X is None:
        return 0
    m = int.from_bytes(bytes(msg32), "big") % N
    sn = pow(sp, -1, N)
    D = pt_add(pt_mul(sn * sigr, X), pt_mul(sn * m, G))
    return int(D is not INF and D == Rp)


def sign(x, Y, msg32, k, k_dleq):
    """a valid adaptor signature of msg32 under the secret key x for the encryption key Y (a point): R = k*Y, R' = k*G,
    s' = (m + x(R) x)/k, and the DLEQ proof (e, s) of log_G R' == log_Y R with the nonce k_dleq"""
    R, Rp = pt_mul(k, Y), pt_mul(k, G)
    e = dleq_challenge(Rp, Y, R, pt_mul(k_dleq, G), pt_mul(k_dleq, Y))
    s = (k_dleq + e * k) % N
    m = int.from_bytes(bytes(msg32), "big") % N
    sp = (m + (R[0] % N) * x) * pow(k, -1, N) % N
    assert sp != 0 and R[0] % N != 0
    return ser33(R) + ser33(Rp) + b32(sp) + b32(e) + b32(s)


def sig_fields(sig):
    return dict(R=sig[0:33], Rp=sig[33:66], sp=int.from_bytes(sig[66:98], "big"), e=int.from_bytes(sig[98:130], "big"), s=int.from_bytes(sig[130:162], "big"))


def sig_pack(R, Rp, sp, e, s):
    return bytes(R) + bytes(Rp) + b32(sp) + b32(e) + b32(s)


# ---- key formats ------------------------------------------------------------------------------------------------------------------------
def key_object(key33, parse=None):
    """the 64-byte secp256k1_pubkey object of a compressed key, or None when it does not parse.  parse: secp256k1_ec_pubkey_parse of the
    reference library (tests.tweak_ref.TweakRef.ec_parse) where there is one; without it the object is written here (x, y as 32
    little-endian bytes each -- the layout the engine documents for pk_format 1)."""
    if parse is not None:
        return parse(bytes(key33))
    a = parse33(bytes(key33))
    return None if a is None else a[0].to_bytes(32, "little") + a[1].to_bytes(32, "little")


def key_full(key33):
    a = parse33(bytes(key33))
    return None if a is None else b"\x04" + a[0].to_bytes(32, "big") + a[1].to_bytes(32, "big")


def keys_in_format(item, fmt, parse=None):
    """(pubkey, enckey) of an item in pk_format fmt, or None when the item does not exist in that format"""
    _, _, pk, _, ek, _, only = item
    if only is not None:
        return (pk, ek) if fmt == only else None
    if fmt == 0:
        return pk, ek
    conv = (lambda k: key_object(k, parse)) if fmt == 1 else key_full
    a, b = conv(pk), conv(ek)
    return None if a is None or b is None else (a, b)


# ---- items ------------------------------------------------------------------------------------------------------------------------------
def _rand_scalar(rng):
    return int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()), "big") % (N - 1) + 1


def _flip(b, bit):
    b = bytearray(b); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)


def make_item(name, sig, pk, msg, ek, verdict=None, fmt_only=None):
    """verdict None: the model's"""
    sig, pk, msg, ek = bytes(sig), bytes(pk), bytes(msg), bytes(ek)
    if verdict is None:
        verdict = verify(sig, pk, msg, ek)
    return (name, sig, pk, msg, ek, int(verdict), fmt_only)


def edge_cases():
    """every item is built from one valid signature; the expected verdicts of the comments are asserted by tests/test_cpu_adaptor.py
    (test_edge_list_verdicts) on the model and were returned by the reference when the fixture was written"""
    rng = np.random.default_rng(5501)
    x, y, k, kd = (_rand_scalar(rng) for _ in range(4))
    X, Y = pt_mul(x, G), pt_mul(y, G)
    msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())
    m = int.from_bytes(msg, "big") % N
    sig = sign(x, Y, msg, k, kd)
    f = sig_fields(sig)
    R, Rp = parse33(f["R"]), parse33(f["Rp"])
    pk, ek = ser33(X), ser33(Y)
    out = []

    def add(name, s=sig, p=pk, mm=msg, e=ek, **kw):
        out.append(make_item(name, s, p, mm, e, **kw))

    add("valid")
    # parsing
    add("s' = 0", sig_pack(f["R"], f["Rp"], 0, f["e"], f["s"]))
    add("s' = n", sig_pack(f["R"], f["Rp"], N, f["e"], f["s"]))
    add("s = n", sig_pack(f["R"], f["Rp"], f["sp"], f["e"], N))
    add("prefix 04 on R", b"\x04" + sig[1:])
    add("x >= p in R'", sig_pack(f["R"], b"\x02" + b32(P + 1), f["sp"], f["e"], f["s"]))
    add("s = 0", sig_pack(f["R"], f["Rp"], f["sp"], f["e"], 0))
    add("e = 0", sig_pack(f["R"], f["Rp"], f["sp"], 0, f["s"]))
    # malleability
    add("s' + 1 (DLEQ passes, ECDSA fails)", sig_pack(f["R"], f["Rp"], f["sp"] + 1, f["e"], f["s"]))
    add("n - s'", sig_pack(f["R"], f["Rp"], N - f["sp"], f["e"], f["s"]))
    add("R' negated", sig_pack(f["R"], ser33(pt_neg(Rp)), f["sp"], f["e"], f["s"]))
    add("R negated", sig_pack(ser33(pt_neg(R)), f["Rp"], f["sp"], f["e"], f["s"]))
    add("n - s' and R' negated", sig_pack(f["R"], ser33(pt_neg(Rp)), N - f["sp"], f["e"], f["s"]))
    add("msg + 1", mm=b32(int.from_bytes(msg, "big") + 1))
    # keys
    add("Y negated", e=ser33(pt_neg(Y)))
    add("X negated", p=ser33(pt_neg(X)))
    add("X and Y swapped", p=ek, e=pk)
    out.append(make_item("all-zero key objects", sig, bytes(64), msg, bytes(64), verdict=0, fmt_only=1))
    out.append(make_item("all-zero pubkey object", sig, bytes(64), msg, key_object(ek), verdict=0, fmt_only=1))
    out.append(make_item("all-zero enckey object", sig, key_object(pk), msg, bytes(64), verdict=0, fmt_only=1))
    # infinity and doubling inside the arithmetic.  R1 = s*G - e*R' with R' = k*G; R2 = s*Y - e*R with R = k2*Y
    e = f["e"]
    add("s = e k: R1 at infinity", sig_pack(f["R"], f["Rp"], f["sp"], e, e * k % N))
    k2 = _rand_scalar(rng)
    R_k2 = ser33(pt_mul(k2, Y))
    add("R = k2 Y, s = e k2: R2 at infinity", sig_pack(R_k2, f["Rp"], f["sp"], e, e * k2 % N))
    add("R = k2 Y, s = -e k2: the doubling inside R2", sig_pack(R_k2, f["Rp"], f["sp"], e, (N - e * k2 % N) % N))
    sigr = R[0] % N
    add("m = -sigr x: D at infinity", mm=b32((N - sigr * x % N) % N))
    add("m = sigr x: the doubling inside D", mm=b32(sigr * x % N))
    # valid items with special keys and messages
    add("Y = G", sign(x, G, msg, k, kd), e=ser33(G))
    add("Y = X", sign(x, X, msg, k, kd), e=pk)
    add("k = 1: R = Y, R' = G", sign(x, Y, msg, 1, kd))
    add("msg = 0", sign(x, Y, bytes(32), k, kd), mm=bytes(32))
    s5 = sign(x, Y, b32(5), k, kd)
    add("msg = 5", s5, mm=b32(5))
    add("msg = n + 5, the signature of msg = 5", s5, mm=b32(N + 5))
    return out


EDGE_VERDICTS = {"valid": 1, "Y = G": 1, "Y = X": 1, "k = 1: R = Y, R' = G": 1, "msg = 0": 1, "msg = 5": 1, "msg = n + 5, the signature of msg = 5": 1}      # every other edge item: 0


def random_items(n, seed, corrupt_every=4):
    """seeded valid items on a few keys; every corrupt_every-th one carries one flipped bit somewhere in its 162 + 33 + 32 + 33 bytes"""
    rng = np.random.default_rng(seed)
    keys = [_rand_scalar(rng) for _ in range(4)]
    out = []
    for i in range(n):
        x = keys[int(rng.integers(0, 4))]; y = _rand_scalar(rng)
        msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())
        sig = sign(x, pt_mul(y, G), msg, _rand_scalar(rng), _rand_scalar(rng))
        pk, ek = ser33(pt_mul(x, G)), ser33(pt_mul(y, G))
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            blob = _flip(sig + pk + msg + ek, int(rng.integers(0, 8 * 260)))
            sig, pk, msg, ek = blob[:162], blob[162:195], blob[195:227], blob[227:260]
        out.append(make_item(f"random {i}", sig, pk, msg, ek))
    return out


def to_json(items):
    return [[nm, sig.hex(), pk.hex(), msg.hex(), ek.hex(), v, only] for nm, sig, pk, msg, ek, v, only in items]


def from_json(rows):
    return [(nm, bytes.fromhex(sig), bytes.fromhex(pk), bytes.fromhex(msg), bytes.fromhex(ek), v, only) for nm, sig, pk, msg, ek, v, only in rows]
