"""A Python statement of secp256k1_ecdsa_s2c_verify_commit, secp256k1_anti_exfil_host_verify and secp256k1_ecdsa_anti_exfil_host_commit over
plain integers (src/modules/ecdsa_s2c/main_impl.h:88-188, src/eccommit_impl.h:16-72 of the reference), a signer for them, and the edge list
the sign-to-contract tests share.  Test-only.

The reference library the other oracles use (oracle/_ref) is built without the ecdsa_s2c module, so this model is the oracle of the CPU
tier; what ties it to the reference is tests/golden/s2c_vectors.json, whose verdicts the reference's own functions returned when
tests/golden/make_s2c_golden.py wrote the file.

An item is the tuple
    (name, sig, msg32, pubkey, data32, opening, commit, host, only)
with the two verdicts (commit, host) and, when only is None, the signature as 64 compact bytes and key and opening as 33 compressed bytes:
keys_in_format() gives them in any format combination of the engine in which the item exists.  only names the one format an item exists in
otherwise: "der" (sig: DER bytes), "obj_sig" (sig: a 64-byte signature object no parser produces), "obj_pubkey" / "obj_opening" (an
all-zero 64-byte object).  The three object kinds carry the engine's contract: the reference calls its illegal-argument callback there
or cannot be handed such an object.  The signer takes the nonce as an argument: how it is derived does not matter to verification."""
import hashlib

import numpy as np

from tests.adaptor_ref import G, INF, N, P, b32, lift_x, parse33, pt_add, pt_mul, pt_neg, ser33  # noqa: F401

TAG_POINT = b"s2c/ecdsa/point"
TAG_DATA = b"s2c/ecdsa/data"


def _tagged(tag, msg):
    t = hashlib.sha256(tag).digest()
    return hashlib.sha256(t + t + msg).digest()


# ---- SHA-256's compression function, for the midstate test --------------------------------------------------------------------------------
def _primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


def _frac_root_bits(p, root):
    """the first 32 bits of the fractional part of p^(1/root), by integer arithmetic"""
    v = p << (32 * root)
    lo, hi = 0, 1 << 40
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** root <= v:
            lo = mid
        else:
            hi = mid - 1
    return lo & 0xFFFFFFFF


SHA_IV = [_frac_root_bits(p, 2) for p in _primes(8)]
SHA_K = [_frac_root_bits(p, 3) for p in _primes(64)]


def sha256_compress(state, block64):
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & 0xFFFFFFFF                        # noqa: E731
    w = [int.from_bytes(block64[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & 0xFFFFFFFF)
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[i] + w[i]) & 0xFFFFFFFF
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xFFFFFFFF
        a, b, c, d, e, f, g, h = (t1 + t2) & 0xFFFFFFFF, a, b, c, (d + t1) & 0xFFFFFFFF, e, f, g
    return [(x + y) & 0xFFFFFFFF for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def tag_midstate(tag):
    """the SHA-256 state after the block SHA256(tag) | SHA256(tag)"""
    t = hashlib.sha256(tag).digest()
    return sha256_compress(SHA_IV, t + t)


# ---- parsers --------------------------------------------------------------------------------------------------------------------------------
def parse_compact(sig64):
    """secp256k1_ecdsa_signature_parse_compact: (r, s), or None when either is >= n"""
    r, s = int.from_bytes(sig64[:32], "big"), int.from_bytes(sig64[32:], "big")
    return None if r >= N or s >= N else (r, s)


def _der_len(b, pos, end):
    if pos >= end:
        return None
    b1 = b[pos]; pos += 1
    if b1 == 0xFF:
        return None
    if b1 & 0x80 == 0:
        return b1, pos
    if b1 == 0x80:
        return None
    k = b1 & 0x7F
    if k > end - pos or b[pos] == 0 or k > 8:
        return None
    ln = int.from_bytes(b[pos:pos + k], "big"); pos += k
    if ln > end - pos or ln < 128:
        return None
    return ln, pos


def _der_int(b, pos, end):
    if pos == end or b[pos] != 0x02:
        return None
    got = _der_len(b, pos + 1, end)
    if got is None:
        return None
    ln, pos = got
    if ln == 0 or ln > end - pos:
        return None
    if b[pos] == 0x00 and ln > 1 and b[pos + 1] & 0x80 == 0:
        return None
    if b[pos] == 0xFF and ln > 1 and b[pos + 1] & 0x80:
        return None
    v = int.from_bytes(b[pos:pos + ln], "big")
    if b[pos] & 0x80 or v >= N:                      # negative, too long or >= n: parses as 0
        v = 0
    return v, pos + ln


def parse_der(sig):
    """secp256k1_ecdsa_signature_parse_der (src/ecdsa_impl.h:141-193): (r, s) or None"""
    sig = bytes(sig)
    if len(sig) == 0 or sig[0] != 0x30:
        return None
    got = _der_len(sig, 1, len(sig))
    if got is None or got[0] != len(sig) - got[1]:
        return None
    a = _der_int(sig, got[1], len(sig))
    if a is None:
        return None
    c = _der_int(sig, a[1], len(sig))
    if c is None or c[1] != len(sig):
        return None
    return a[0], c[0]


def der_encode(r, s):
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        return b"\x02" + bytes([len(b) + (b[0] >> 7)]) + (b"\0" if b[0] & 0x80 else b"") + b
    body = integer(r) + integer(s)
    assert len(body) < 128
    return b"\x30" + bytes([len(body)]) + body


# ---- the verifiers and a signer -------------------------------------------------------------------------------------------------------------
def s2c_tweak(opening_pt, data32):
    return int.from_bytes(_tagged(TAG_POINT, ser33(opening_pt) + bytes(data32)), "big")


def commit_rs(rs, data32, opening_pt):
    """rs: the parsed signature or None; opening_pt: the loaded opening or None"""
    if rs is None or opening_pt is None:
        return 0
    t = s2c_tweak(opening_pt, data32)
    if t >= N:
        return 0
    R = pt_add(opening_pt, pt_mul(t, G))
    return int(R is not INF and R[0] % N == rs[0])


def ecdsa_rs(rs, msg32, key_pt):
    if rs is None or key_pt is None:
        return 0
    r, s = rs
    if r == 0 or s == 0 or s > N // 2:
        return 0
    m = int.from_bytes(bytes(msg32), "big") % N
    sn = pow(s, -1, N)
    R = pt_add(pt_mul(sn * m, G), pt_mul(sn * r, key_pt))
    return int(R is not INF and R[0] % N == r)


def verify_commit(sig64, data32, opening33):
    """compact signature, compressed opening; returns 0 or 1"""
    return commit_rs(parse_compact(bytes(sig64)), data32, parse33(bytes(opening33)))


def host_verify(sig64, msg32, pubkey33, host_data32, opening33):
    rs = parse_compact(bytes(sig64))
    return commit_rs(rs, host_data32, parse33(bytes(opening33))) & ecdsa_rs(rs, msg32, parse33(bytes(pubkey33)))


def host_commit(rand32):
    return _tagged(TAG_DATA, bytes(rand32))


def sign(d, msg32, k, data32):
    """-> (compact signature, opening33): opening k*G, t = H(k*G, data), r = x((k + t)*G) mod n, s = (m + r d)/(k + t), low s"""
    O = pt_mul(k, G)
    kk = (k + s2c_tweak(O, data32)) % N
    r = pt_mul(kk, G)[0] % N
    s = (int.from_bytes(bytes(msg32), "big") + r * d) * pow(kk, -1, N) % N
    assert r != 0 and s != 0
    return b32(r) + b32(min(s, N - s)), ser33(O)


def sign_plain(d, msg32, k):
    r = pt_mul(k, G)[0] % N
    s = (int.from_bytes(bytes(msg32), "big") + r * d) * pow(k, -1, N) % N
    return b32(r) + b32(min(s, N - s))


# ---- formats --------------------------------------------------------------------------------------------------------------------------------
def key_object(key33):
    """the 64-byte secp256k1_pubkey / secp256k1_ecdsa_s2c_opening object of a compressed point, or None when it does not parse"""
    a = parse33(bytes(key33))
    return None if a is None else a[0].to_bytes(32, "little") + a[1].to_bytes(32, "little")


def key_full(key33):
    a = parse33(bytes(key33))
    return None if a is None else b"\x04" + b32(a[0]) + b32(a[1])


def sig_object(sig64):
    """the 64-byte secp256k1_ecdsa_signature object of a compact signature, or None when it does not parse"""
    rs = parse_compact(bytes(sig64))
    return None if rs is None else rs[0].to_bytes(32, "little") + rs[1].to_bytes(32, "little")


def keys_in_format(item, sig_format, pk_format, opening_format):
    """(sig, pubkey, opening) of an item in this format combination, or None when the item does not exist in it"""
    _, sig, _, pk, _, op, _, _, only = item
    if only == "der":
        sig = sig if sig_format == 2 else None
    elif only == "obj_sig":
        sig = sig if sig_format == 1 else None
    elif sig_format == 1:
        sig = sig_object(sig)
    elif sig_format == 2:
        rs = parse_compact(sig)
        sig = None if rs is None else der_encode(*rs)
    if only == "obj_pubkey":
        pk = pk if pk_format == 1 else None
    elif pk_format:
        pk = key_object(pk) if pk_format == 1 else key_full(pk)
    if only == "obj_opening":
        op = op if opening_format == 1 else None
    elif opening_format:
        op = key_object(op)
    return None if sig is None or pk is None or op is None else (sig, pk, op)


FORMAT_COMBINATIONS = [(sf, pf, of) for sf in (0, 1, 2) for pf in (0, 1, 2) for of in (0, 1)]


# ---- items ----------------------------------------------------------------------------------------------------------------------------------
def _rand_scalar(rng):
    return int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()), "big") % (N - 1) + 1


def _rand32(rng):
    return bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())


def _flip(b, bit):
    b = bytearray(b); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)


def make_item(name, sig, msg, pk, data, op, verdicts=None, only=None):
    """verdicts None: the model's"""
    sig, msg, pk, data, op = bytes(sig), bytes(msg), bytes(pk), bytes(data), bytes(op)
    if verdicts is None:
        rs = parse_der(sig) if only == "der" else parse_compact(sig)
        c = commit_rs(rs, data, parse33(op))
        verdicts = (c, c & ecdsa_rs(rs, msg, parse33(pk)))
    return (name, sig, msg, pk, data, op, int(verdicts[0]), int(verdicts[1]), only)


def off_curve_x():
    x = 5
    while lift_x(x, 0) is not None:
        x += 1
    return x


def edge_cases():
    """every item is built from one valid signature; the verdicts its name promises (EDGE_VERDICTS) are asserted by tests/test_cpu_s2c.py
    on the model and were returned by the reference when the fixture was written"""
    rng = np.random.default_rng(5601)
    d, k, d2, k2 = (_rand_scalar(rng) for _ in range(4))
    msg, data, msg2, data2 = (_rand32(rng) for _ in range(4))
    X = pt_mul(d, G); pk = ser33(X)
    sig, op = sign(d, msg, k, data)
    sig2, op2 = sign(d2, msg2, k2, data2)
    r, s = parse_compact(sig)
    O = parse33(op)
    out = []

    def add(name, sg=sig, mm=msg, p=pk, dd=data, o=op, **kw):
        out.append(make_item(name, sg, mm, p, dd, o, **kw))

    add("valid")
    add("one data bit flipped", dd=_flip(data, 77))
    add("opening negated", o=ser33(pt_neg(O)))
    add("opening of another item", o=op2)
    add("opening with prefix 04", o=b"\x04" + op[1:])
    add("opening with prefix 00", o=b"\x00" + op[1:])
    add("opening with x >= p", o=b"\x02" + b32(P + 1))
    add("opening with x not on the curve", o=b"\x02" + b32(off_curve_x()))
    add("all-zero opening object", o=bytes(64), verdicts=(0, 0), only="obj_opening")
    add("r + 1", sg=b32(r + 1) + sig[32:])
    add("r = 0", sg=b32(0) + sig[32:])
    add("r >= n in compact form", sg=b32(N) + sig[32:])
    add("s >= n in compact form", sg=sig[:32] + b32(N + 1))
    add("object limbs >= n: r", sg=N.to_bytes(32, "little") + s.to_bytes(32, "little"), verdicts=(0, 0), only="obj_sig")
    add("object limbs >= n: s", sg=r.to_bytes(32, "little") + (N + 1).to_bytes(32, "little"), verdicts=(0, 0), only="obj_sig")
    add("s -> n - s", sg=sig[:32] + b32(N - s))
    add("s = 0", sg=sig[:32] + b32(0))
    add("message + 1", mm=b32(int.from_bytes(msg, "big") + 1))
    add("public key negated", p=ser33(pt_neg(X)))
    add("public key unparsable", p=b"\x05" + pk[1:])
    add("all-zero public-key object", p=bytes(64), verdicts=(1, 0), only="obj_pubkey")
    add("valid plain ECDSA signature with an unrelated opening", sg=sign_plain(d, msg, k2))
    add("another valid item", sg=sig2, mm=msg2, p=ser33(pt_mul(d2, G)), dd=data2, o=op2)
    add("valid DER signature", sg=der_encode(r, s), only="der")
    add("DER signature with a trailing byte", sg=der_encode(r, s) + b"\0", only="der")
    add("DER signature whose r is >= n (parses as 0)", sg=der_encode(r + N if r + N < 1 << 256 else N, s), only="der")
    return out


# (commit, host) of every edge item that is not (0, 0)
EDGE_VERDICTS = {"valid": (1, 1), "another valid item": (1, 1), "valid DER signature": (1, 1), "s -> n - s": (1, 0), "s = 0": (1, 0), "message + 1": (1, 0),
                 "public key negated": (1, 0), "public key unparsable": (1, 0), "all-zero public-key object": (1, 0)}


def random_items(n, seed, corrupt_every=4):
    """seeded valid items on a few keys; every corrupt_every-th one carries one flipped bit somewhere in its 64 + 32 + 33 + 32 + 33 bytes"""
    rng = np.random.default_rng(seed)
    keys = [_rand_scalar(rng) for _ in range(4)]
    out = []
    for i in range(n):
        d = keys[int(rng.integers(0, 4))]
        msg, data = _rand32(rng), _rand32(rng)
        sig, op = sign(d, msg, _rand_scalar(rng), data)
        pk = ser33(pt_mul(d, G))
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            blob = _flip(sig + msg + pk + data + op, int(rng.integers(0, 8 * 194)))
            sig, msg, pk, data, op = blob[:64], blob[64:96], blob[96:129], blob[129:161], blob[161:194]
        out.append(make_item(f"random {i}", sig, msg, pk, data, op))
    return out


def x_above_n_cases(seed=5605):
    """(name, x | y, z, r, expected) for s2c_x_matches on the point (x z^2, y z^3, z).  No entry point reaches x(R) >= n (it needs a fixed
    point of the hash), so the branch r + n is met here: the smallest k with x = n + k on the curve, with r = k (1) and r = k + 1 (0);
    next to it small x < p - n with r = x, which match in the first branch, and r = x + 1, which match in neither."""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    while lift_x(N + k, 0) is None:
        k += 1
    assert N + k < P
    for odd in (0, 1):
        pt = lift_x(N + k, odd)
        for _ in range(2):
            z = _rand_scalar(rng) % P or 1
            out.append((f"x = n + {k}, r = {k}", b32(pt[0]) + b32(pt[1]), b32(z), b32(k), 1))
            out.append((f"x = n + {k}, r = {k + 1}", b32(pt[0]) + b32(pt[1]), b32(z), b32(k + 1), 0))
            out.append((f"x = n + {k}, r = x - n - 1", b32(pt[0]) + b32(pt[1]), b32(z), b32((k - 1) % N), 0))
    small = [x for x in range(1, 40) if lift_x(x, 0) is not None][:4]
    for x in small:
        pt = lift_x(x, x & 1)
        z = _rand_scalar(rng) % P or 1
        out.append((f"x = {x}, r = x", b32(pt[0]) + b32(pt[1]), b32(z), b32(x), 1))
        out.append((f"x = {x}, r = x + 1", b32(pt[0]) + b32(pt[1]), b32(z), b32(x + 1), 0))
    for i in range(4):
        pt = pt_mul(_rand_scalar(rng), G)
        z = 1 if i == 0 else _rand_scalar(rng) % P or 1
        out.append((f"random point {i}, r = x mod n", b32(pt[0]) + b32(pt[1]), b32(z), b32(pt[0] % N), 1))
        out.append((f"random point {i}, r = x mod n + 1", b32(pt[0]) + b32(pt[1]), b32(z), b32((pt[0] + 1) % N), 0))
    return out


def to_json(items):
    return [[nm, sig.hex(), msg.hex(), pk.hex(), data.hex(), op.hex(), c, h, only] for nm, sig, msg, pk, data, op, c, h, only in items]


def from_json(rows):
    return [(nm, bytes.fromhex(sig), bytes.fromhex(msg), bytes.fromhex(pk), bytes.fromhex(data), bytes.fromhex(op), c, h, only)
            for nm, sig, msg, pk, data, op, c, h, only in rows]
