"""Plain-Python model of the ElligatorSwift routines the engine serves (BIP-324; the reference's src/modules/ellswift/main_impl.h):
decode (secp256k1_ellswift_decode :470-483 over xswiftec_frac_var :24-132), the partial inverse (xswiftec_inv_var :168-303) and the
encode loop (secp256k1_ellswift_encode :393-420 over xelligatorswift_var :333-367).  Nothing here is fast and nothing is shared with
csrc/ellswift.h: integers mod p and hashlib.  tests/golden/make_ellswift_golden.py checks it against the reference before it writes
tests/golden/ellswift_vectors.json; the CPU and GPU tests check the engine against that file and against this model."""
import hashlib
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
# c1 = (sqrt(-3) - 1) / 2 with the root the reference fixed (:14-21); c2 = -c1 - 1, c3 = -c1, c4 = c1 + 1
C1 = 0x851695d49a83f8ef919bb86153cbcb16630fb68aed0a766a3ec693d68e6afa40
C2 = (-C1 - 1) % P
C3 = (-C1) % P
C4 = (C1 + 1) % P
assert (2 * C1 + 1) ** 2 % P == P - 3
MAX_ATTEMPTS = 256          # the engine's cap (the reference loops until it succeeds)


def fe_sqrt(a):
    """the root the reference's secp256k1_fe_sqrt returns, a^((p+1)/4), or None"""
    a %= P
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a else None


def is_square(a):
    """secp256k1_fe_is_square_var: 0 counts"""
    return fe_sqrt(a) is not None


def on_curve_frac(n, d):
    """n / d is the x of a point: (n^3 + 7 d^3) d is a square (secp256k1_ge_x_frac_on_curve_var)"""
    return is_square((pow(n, 3, P) + 7 * pow(d, 3, P)) * d)


def xswiftec_frac(u, t):
    """-> (xn, xd, which) with which = 3, 2, 1 for x3, x2, x1; u, t any integers (reduced here)"""
    u %= P; t %= P
    if u == 0:
        u = 1
    s = t * t % P if t else 1
    g = (u * u * u + 7) % P
    if (g + s) % P == 0:
        s = 4 * s % P
    p = (g + s) % P
    d = 3 * s * u * u % P
    n = (d * u - p * p) % P
    if on_curve_frac(n, d):
        return n, d, 3
    n = u * (C1 * s + C2 * g) % P
    if on_curve_frac(n, p):
        return n, p, 2
    n = (-(n + u * p)) % P
    assert on_curve_frac(n, p)
    return n, p, 1


def xswiftec(u, t):
    n, d, which = xswiftec_frac(u, t)
    return n * pow(d, P - 2, P) % P, which


def g_plus_s_zero(u, t):
    """does (u, t) take the s <- 4 s substitution?"""
    u %= P; t %= P
    if u == 0:
        u = 1
    s = t * t % P if t else 1
    return (u * u * u + 7 + s) % P == 0


def decode(ell64):
    """-> (x, y, which): secp256k1_ellswift_decode.  The parity of y is that of t reduced mod p."""
    u = int.from_bytes(ell64[:32], "big"); t = int.from_bytes(ell64[32:], "big") % P
    x, which = xswiftec(u, t)
    y = fe_sqrt(x * x * x + 7)
    assert y is not None
    if (y & 1) != (t & 1):
        y = P - y
    return x, y, which


def pubkey_object(x, y):
    """the 64-byte secp256k1_pubkey object on a little-endian machine: x | y, each as 32 little-endian bytes"""
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def ser33(x, y):
    return bytes([2 + (y & 1)]) + x.to_bytes(32, "big")


def decode_out(ell64, out_format):
    x, y, _ = decode(ell64)
    return x.to_bytes(32, "big") if out_format == 0 else pubkey_object(x, y) if out_format == 1 else ser33(x, y)


def xswiftec_inv(x, u, c):
    """-> t or None: secp256k1_ellswift_xswiftec_inv_var.  x on the curve, u != 0."""
    x %= P; u %= P
    g = (u * u * u + 7) % P
    if not c & 2:
        m = (-u - x) % P
        if is_square(m * m * m + 7):
            return None
        s = (-(u * u + u * x + x * x)) % P
        if not is_square(s * g):
            return None
        s = g * pow(s, P - 2, P) % P
        v = x
    else:
        s = (x - u) % P
        if not is_square(s):
            return None
        r = fe_sqrt(-s * (4 * g + 3 * s * u * u))
        if r is None:
            return None
        if (c & 1) and r == 0:
            return None
        if s == 0:
            return None
        v = (r * pow(s, P - 2, P) - u) * pow(2, P - 2, P) % P
    w = fe_sqrt(s)
    assert w is not None
    if (c & 5) in (0, 5):
        w = P - w
    return w * ((C4 if c & 1 else C3) * u + v) % P


def tag_prefix():
    th = hashlib.sha256(b"secp256k1_ellswift_encode").digest()
    return th + th


def draw_counter(attempt):
    """the counter whose hash is u of attempt `attempt` (from 0): every 65th counter refills the branch pool"""
    return attempt + attempt // 64 + 1


def pool_counter(attempt):
    return 65 * (attempt // 64)


def branch_index(attempt):
    """-> (byte of the pool hash, shift): branch = (h[byte] >> shift) & 7"""
    k = 63 - attempt % 64
    return k >> 1, (k & 1) << 2


def branch_value(pool_hash, attempt):
    b, sh = branch_index(attempt)
    return (pool_hash[b] >> sh) & 7


def key_parse33(key33):
    """secp256k1_ec_pubkey_parse of 33 bytes -> (x, y) or None"""
    if len(key33) != 33 or key33[0] not in (2, 3):
        return None
    x = int.from_bytes(key33[1:], "big")
    if x >= P:
        return None
    y = fe_sqrt(x * x * x + 7)
    if y is None:
        return None
    if (y & 1) != (key33[0] & 1):
        y = P - y
    return x, y


def encode_point(x, y, rnd32, max_attempts=MAX_ATTEMPTS):
    """-> (ell64 or None, attempts, branch): the reference's loop, cut at max_attempts"""
    base = tag_prefix() + ser33(x, y) + bytes(31) + bytes(rnd32)

    def draw(cnt):
        return hashlib.sha256(base + cnt.to_bytes(4, "little")).digest()
    pool = None
    for a in range(max_attempts):
        if a % 64 == 0:
            pool = draw(pool_counter(a))
        c = branch_value(pool, a)
        u32 = draw(draw_counter(a))
        u = int.from_bytes(u32, "big") % P
        t = xswiftec_inv(x, u, c) if u else None
        if t is not None:
            if (t & 1) != (y & 1):
                t = P - t
            return u32 + t.to_bytes(32, "big"), a + 1, c
    return None, max_attempts, -1


def encode(key, key_format, rnd32, max_attempts=MAX_ATTEMPTS):
    """key_format 1: 64-byte object, 2: 33 bytes compressed -> (result, ell64, attempts, branch); a refused key: (0, 64 zero bytes, 0, -1)"""
    if key_format == 1:
        x = int.from_bytes(key[:32], "little"); y = int.from_bytes(key[32:], "little")
        pt = None if x % P == 0 else (x % P, y % P)
    else:
        pt = key_parse33(key)
    if pt is None:
        return 0, bytes(64), 0, -1
    ell, att, c = encode_point(pt[0], pt[1], rnd32, max_attempts)
    return (1, ell, att, c) if ell is not None else (0, bytes(64), att, -1)


def rounds_per_wavefront(attempts, wave=64):
    """mean over the wavefronts of a batch of the largest attempt count among their items: what the one-item-per-lane loop runs"""
    groups = [attempts[i:i + wave] for i in range(0, len(attempts), wave)]
    return sum(max(g) for g in groups) / len(groups)


# ---- items of the golden file ---------------------------------------------------------------------------------------------------------
def _b(v):
    return (v % 2**256).to_bytes(32, "big")


def decode_edges():
    """[(name, ell64)]: u and t at 0, p, p + 1, 2^256 - 1, odd and even t, a g + s = 0 item, and seeded items until each of x3, x2, x1 is hit
    at least four times"""
    out = []
    special = [("0", 0), ("p", P), ("p+1", P + 1), ("2^256-1", 2**256 - 1)]
    for un, u in special:
        for tn, t in special:
            out.append(("u=%s t=%s" % (un, tn), _b(u) + _b(t)))
    rng = random.Random(324)
    for un, u in special:
        out.append(("u=%s t odd" % un, _b(u) + _b(rng.randrange(P) | 1)))
        out.append(("u=%s t even" % un, _b(u) + _b(rng.randrange(P) & ~1)))
    for tn, t in special:
        out.append(("u random t=%s" % tn, _b(rng.randrange(P)) + _b(t)))
    # g + s = 0: t^2 = -(u^3 + 7)
    while True:
        u = rng.randrange(1, P)
        t = fe_sqrt(-(u * u * u + 7))
        if t:
            break
    assert g_plus_s_zero(u, t)
    out.append(("g+s=0", _b(u) + _b(t)))
    out.append(("g+s=0, -t", _b(u) + _b(P - t)))
    out.append(("g+s=0, t+p", _b(u) + _b(t + P)) if t + P < 2**256 else ("g+s=0 again", _b(u) + _b(t)))
    hits = {1: 0, 2: 0, 3: 0}
    while min(hits.values()) < 4:
        e = _b(rng.randrange(2**256)) + _b(rng.randrange(2**256))
        w = decode(e)[2]
        if hits[w] < 6:
            hits[w] += 1
            out.append(("random, x%d" % w, e))
    return out


def pt_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        l = 3 * a[0] * a[0] * pow(2 * a[1], P - 2, P) % P
    else:
        l = (b[1] - a[1]) * pow(b[0] - a[0], P - 2, P) % P
    x = (l * l - a[0] - b[0]) % P
    return x, (l * (a[0] - x) - a[1]) % P


G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def pt_mul(k, p):
    r = None
    while k:
        if k & 1:
            r = pt_add(r, p)
        p = pt_add(p, p); k >>= 1
    return r


def encode_item_secrets(rng):
    """the secret keys behind the eight public keys of encode_items (tests sign with them); advances rng as encode_items does"""
    return [rng.randrange(1, N) for _ in range(8)]


def ecdsa_sign(d, msg32, k):
    """-> 64 bytes compact r | s (low s), nonce k"""
    r = pt_mul(k, G)[0] % N
    s = pow(k, N - 2, N) * (int.from_bytes(msg32, "big") + r * d) % N
    assert r and s
    return r.to_bytes(32, "big") + min(s, N - s).to_bytes(32, "big")


def encode_items(count=64, seed=3240):
    """[(name, key33, rnd32)]: `count` seeded pairs, rnd32 searched so that every branch value 0..7 is the successful one at least once,
    one item succeeds on its first attempt and one needs at least 12"""
    rng = random.Random(seed)
    keys = [pt_mul(d, G) for d in encode_item_secrets(rng)]
    out, seen, first, long_ = [], set(), False, False
    while len(out) < count:
        x, y = keys[len(out) % len(keys)]
        rnd = bytes(rng.randrange(256) for _ in range(32))
        _, att, c = encode_point(x, y, rnd)
        left = count - len(out)
        missing = (8 - len(seen)) + (not first) + (not long_)
        useful = (c not in seen) or (att == 1 and not first) or (att >= 12 and not long_)
        if left <= missing and not useful:
            continue
        seen.add(c); first |= att == 1; long_ |= att >= 12
        out.append(("seeded %d" % len(out), ser33(x, y), rnd))
    assert len(seen) == 8 and first and long_
    return out


def refused_keys():
    """[(name, key bytes, key_format)]: what secp256k1_ec_pubkey_parse refuses in 33 bytes, and the all-zero object"""
    x = G[0]
    off = next(v for v in range(1, 100) if fe_sqrt(v * v * v + 7) is None)
    return [("prefix 04", b"\x04" + _b(x), 2), ("prefix 05", b"\x05" + _b(x), 2), ("x = p", b"\x02" + _b(P), 2), ("x = p + 1", b"\x03" + _b(P + 1), 2),
            ("x off the curve", b"\x02" + _b(off), 2), ("all-zero object", bytes(64), 1)]
