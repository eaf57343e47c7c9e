"""ctypes view of the reference's public-key group in oracle/_ref/libsecp256k1_ref.so (include/secp256k1.h: secp256k1_ec_pubkey_parse,
_serialize, _negate, _tweak_mul, _combine; include/secp256k1_extrakeys.h: secp256k1_xonly_pubkey_parse, _serialize, _from_pubkey) and the
edge lists the public-key tests share.  Test-only.  Every expected verdict and output is the reference's own, asked when the lists are
built.  The exceptions are the engine's documented differences, where the reference is not asked because it would call its
illegal-argument callback: the all-zero key object and the empty set (verdict 0), and a set with a key that does not load (verdict 0).

Formats are the engine's S2K_PK_*: 0 x-only (32 bytes), 1 object (64), 2 compressed (33), 3 uncompressed / hybrid (65), 4 x | y
big-endian (64; defined as the uncompressed serialisation without its prefix byte), 5 x-only object (64, output only).

Items are tuples:
    convert    (name, in_format, key, verdict, outs, parity, neg_outs, neg_parity)
    tweak_mul  (name, key_format, key, tweak32, verdict, outs, parity)
    combine    (name, key_format, keys, verdict, outs, parity)             keys: a list of byte strings
outs: the six output encodings of the result, in format order (zero bytes where the verdict is 0); parity: is_odd(y) of the result."""
import ctypes

import numpy as np

from tests.refapi import REF_PATH, N, P  # noqa: F401

CONTEXT_NONE = 1
EC_COMPRESSED = (1 << 1) | (1 << 8)
EC_UNCOMPRESSED = 1 << 1
PK_BYTES = {0: 32, 1: 64, 2: 33, 3: 65, 4: 64, 5: 64}
IN_FORMATS = (0, 1, 2, 3, 4)
OUT_FORMATS = (0, 1, 2, 3, 4, 5)
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72      # src/scalar_impl.h:83-86
FANIN = 16                                                                          # the first pass's default chunk length

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class PubkeyRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_ec_pubkey_parse": [_vp, _vp, _vp, _sz],
            "secp256k1_ec_pubkey_serialize": [_vp, _vp, _vp, _vp, ctypes.c_uint],
            "secp256k1_ec_pubkey_negate": [_vp, _vp],
            "secp256k1_ec_pubkey_tweak_mul": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_combine": [_vp, _vp, _vp, _sz],
            "secp256k1_xonly_pubkey_parse": [_vp, _vp, _vp],
            "secp256k1_xonly_pubkey_serialize": [_vp, _vp, _vp],
            "secp256k1_xonly_pubkey_from_pubkey": [_vp, _vp, _vp, _vp],
            "secp256k1_ec_pubkey_create": [_vp, _vp, _vp],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx

    # ---- the eight calls (and secp256k1_ec_pubkey_create, for making keys); key objects are 64 bytes ---------------------------------------
    def ec_parse(self, ser):
        o = ctypes.create_string_buffer(b"\xff" * 64, 64)
        if self.lib.secp256k1_ec_pubkey_parse(self.ctx, o, bytes(ser), len(ser)) == 1:
            return o.raw
        assert o.raw == bytes(64)
        return None

    def ec_serialize(self, obj64, compressed=True):
        n = 33 if compressed else 65
        o = ctypes.create_string_buffer(n); ln = _sz(n)
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, o, ctypes.byref(ln), bytes(obj64), EC_COMPRESSED if compressed else EC_UNCOMPRESSED) == 1 and ln.value == n
        return o.raw

    def ec_negate(self, obj64):
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        assert self.lib.secp256k1_ec_pubkey_negate(self.ctx, o) == 1
        return o.raw

    def ec_tweak_mul(self, obj64, tweak32):
        """-> the product's object, or None (the reference zeroes the object then)"""
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        if self.lib.secp256k1_ec_pubkey_tweak_mul(self.ctx, o, bytes(tweak32)) == 1:
            return o.raw
        assert o.raw == bytes(64)
        return None

    def ec_combine(self, objs):
        """-> the sum's object, or None; at least one key"""
        assert len(objs) >= 1
        bufs = [ctypes.create_string_buffer(bytes(x), 64) for x in objs]
        ptrs = (_vp * len(bufs))(*[ctypes.addressof(b) for b in bufs])
        o = ctypes.create_string_buffer(b"\xff" * 64, 64)
        if self.lib.secp256k1_ec_pubkey_combine(self.ctx, o, ptrs, len(bufs)) == 1:
            return o.raw
        assert o.raw == bytes(64)
        return None

    def xonly_parse(self, x32):
        o = ctypes.create_string_buffer(b"\xff" * 64, 64)
        if self.lib.secp256k1_xonly_pubkey_parse(self.ctx, o, bytes(x32)) == 1:
            return o.raw
        assert o.raw == bytes(64)
        return None

    def xonly_serialize(self, xobj64):
        o = ctypes.create_string_buffer(32)
        assert self.lib.secp256k1_xonly_pubkey_serialize(self.ctx, o, bytes(xobj64)) == 1
        return o.raw

    def xonly_from_pubkey(self, obj64):
        o = ctypes.create_string_buffer(64); par = _int(-1)
        assert self.lib.secp256k1_xonly_pubkey_from_pubkey(self.ctx, o, ctypes.byref(par), bytes(obj64)) == 1
        return o.raw, par.value

    def ec_create(self, seckey32):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ec_pubkey_create(self.ctx, o, bytes(seckey32)) == 1
        return o.raw

    # ---- what the engine's calls are compared with --------------------------------------------------------------------------------------
    def load(self, fmt, key):
        """a key in an input format -> its object, or None where the format's parser refuses it"""
        key = bytes(key)
        assert len(key) == PK_BYTES[fmt] and fmt in IN_FORMATS
        if fmt == 0:
            return self.xonly_parse(key)
        if fmt == 1:
            return None if key[:32] == bytes(32) else key
        if fmt == 4:
            return self.ec_parse(b"\x04" + key)
        return self.ec_parse(key)

    def outs(self, obj64):
        """an object (None: refused) -> (the six output encodings, parity)"""
        if obj64 is None:
            return tuple(bytes(PK_BYTES[f]) for f in OUT_FORMATS), 0
        xobj, par = self.xonly_from_pubkey(obj64)
        full = self.ec_serialize(obj64, False)
        return (self.xonly_serialize(xobj), bytes(obj64), self.ec_serialize(obj64, True), full, full[1:], xobj), par

    def encode(self, obj64, fmt):
        """an object in input format fmt (0 drops the parity of y)"""
        return self.outs(obj64)[0][fmt]


def b32(v):
    return int(v).to_bytes(32, "big")


def _seckey(rng):
    return bytes(rng.integers(0, 256, 31, dtype=np.uint8).tolist()) + b"\x01"


def convert_item(ref, name, fmt, key):
    obj = ref.load(fmt, key)
    o, p = ref.outs(obj)
    no, np_ = ref.outs(None if obj is None else ref.ec_negate(obj))
    return (name, fmt, bytes(key), int(obj is not None), o, p, no, np_)


def tweak_mul_item(ref, name, fmt, key, tweak32):
    obj = ref.load(fmt, key)
    o, p = ref.outs(None if obj is None else ref.ec_tweak_mul(obj, tweak32))
    return (name, fmt, bytes(key), bytes(tweak32), int(any(o[1])), o, p)


def combine_item(ref, name, fmt, keys):
    objs = [ref.load(fmt, k) for k in keys]
    res = None if (not objs or any(x is None for x in objs)) else ref.ec_combine(objs)
    o, p = ref.outs(res)
    return (name, fmt, [bytes(k) for k in keys], int(res is not None), o, p)


def _hybrid(full65):
    return bytes([6 + (full65[64] & 1)]) + full65[1:]


def convert_edges(ref):
    rng = np.random.default_rng(7701)
    out = []

    def add(name, fmt, key):
        out.append(convert_item(ref, name, fmt, key))

    keys = [ref.ec_create(_seckey(rng)) for _ in range(64)]
    even = next(k for k in keys if k[32] & 1 == 0); odd = next(k for k in keys if k[32] & 1 == 1)
    for nm, obj in (("even y", even), ("odd y", odd)):
        for fmt in IN_FORMATS:
            add(f"valid {nm} fmt {fmt}", fmt, ref.encode(obj, fmt))
        add(f"valid {nm} hybrid", 3, _hybrid(ref.encode(obj, 3)))
    add("object with odd y (to format 5: y is made even)", 1, odd)
    add("all-zero object", 1, bytes(64))
    x_off = next(x for x in range(2, 100) if ref.xonly_parse(b32(x)) is None)
    xs = (("x = p", P), ("x = p - 1", P - 1), ("x = 0", 0), ("x = p + 1", P + 1), ("x = 2^256 - 1", (1 << 256) - 1), ("x = 2^255", 1 << 255),
          (f"x = {x_off} not on the curve", x_off))
    for nm, x in xs:
        add("fmt 0 " + nm, 0, b32(x))
        add("fmt 2 prefix 02 " + nm, 2, b"\x02" + b32(x))
        add("fmt 2 prefix 03 " + nm, 2, b"\x03" + b32(x))
    ser = ref.encode(even, 2); full = ref.encode(odd, 3); full_e = ref.encode(even, 3)
    for pfx in (0x00, 0x01, 0x04, 0x05, 0x06, 0x07):
        add(f"fmt 2 bad prefix {pfx:02x}", 2, bytes([pfx]) + ser[1:])
    for pfx in (0x00, 0x02, 0x03, 0x05, 0x08):
        add(f"fmt 3 bad prefix {pfx:02x}", 3, bytes([pfx]) + full[1:])
    add("fmt 3 prefix 06 with odd y", 3, b"\x06" + full[1:])
    add("fmt 3 prefix 07 with odd y", 3, b"\x07" + full[1:])
    add("fmt 3 prefix 07 with even y", 3, b"\x07" + full_e[1:])
    add("fmt 3 prefix 06 with even y", 3, b"\x06" + full_e[1:])
    y = int.from_bytes(full[33:], "big")
    for fmt, head in ((3, full[:33]), (4, full[1:33])):
        add(f"fmt {fmt} y = p", fmt, head + b32(P))
        add(f"fmt {fmt} y = 2^256 - 1", fmt, head + b32((1 << 256) - 1))
        add(f"fmt {fmt} y off the curve", fmt, head + b32(y ^ 2))
        add(f"fmt {fmt} y replaced by p - y", fmt, head + b32(P - y))
        add(f"fmt {fmt} y = 0", fmt, head + bytes(32))
    for nm, x in xs[:5]:
        add("fmt 4 " + nm, 4, b32(x) + full[33:])
        add("fmt 3 " + nm, 3, b"\x04" + b32(x) + full[33:])
    assert 0 < sum(x[3] for x in out) < len(out)
    return out


TWEAKS = (("0", 0), ("1", 1), ("2", 2), ("n-1", N - 1), ("n", N), ("n+1", N + 1), ("2^256-1", (1 << 256) - 1), ("lambda", LAMBDA), ("2^128", 1 << 128),
          ("n - lambda", N - LAMBDA), ("2^128 - 1", (1 << 128) - 1))


def tweak_mul_edges(ref):
    rng = np.random.default_rng(7702)
    out = []
    keys = [ref.ec_create(_seckey(rng)) for _ in range(3)]
    for j, obj in enumerate(keys[:1]):
        for fmt in IN_FORMATS:
            for nm, t in TWEAKS:
                out.append(tweak_mul_item(ref, f"key {j} fmt {fmt} tweak {nm}", fmt, ref.encode(obj, fmt), b32(t)))
    t = _seckey(rng)
    bad = [x for x in convert_edges(ref) if x[3] == 0]
    for name, fmt, key, *_ in bad[::3]:
        out.append(tweak_mul_item(ref, "refused key: " + name, fmt, key, t))
    assert 0 < sum(x[4] for x in out) < len(out)
    return out


def combine_edges(ref, fanin=FANIN):
    rng = np.random.default_rng(7703)
    F = fanin
    out = []
    base = [ref.ec_create(_seckey(rng)) for _ in range(2 * F + 1)]
    pool = [base[i % len(base)] for i in range(F * F + 1)]      # (2F + 1 distinct keys, cycled: no chunk of F holds a key twice)
    neg = ref.ec_negate

    def add(name, objs, fmt=1):
        out.append(combine_item(ref, name, fmt, [o if fmt == 1 else ref.encode(o, fmt) for o in objs]))

    for m in sorted({0, 1, 2, 3, F - 1, F, F + 1, 2 * F + 1, F * F + 1} | set(range(1, 10))):
        add(f"{m} keys", pool[:m])
    Pk, Q = pool[0], pool[1]
    PQ = ref.ec_combine([Pk, Q])
    add("[P, P]", [Pk, Pk])
    add("[P, Q, P+Q]", [Pk, Q, PQ])
    add("[P, -P]", [Pk, neg(Pk)])
    add("[P, -P, Q]", [Pk, neg(Pk), Q])
    add("[P, Q, -(P+Q)]", [Pk, Q, neg(PQ)])
    add("[P, P, P, P]", [Pk] * 4)
    add("2F keys, the second chunk repeats the first", pool[:F] + pool[:F])
    add("2F keys, the second chunk negates the first", pool[:F] + [neg(x) for x in pool[:F]])
    add("2F + 1 keys, the second chunk negates the first", pool[:F] + [neg(x) for x in pool[:F]] + [Q])
    for fmt in (0, 2, 3, 4):
        for m in (1, 2, 3, F + 1):
            add(f"{m} keys fmt {fmt}", pool[:m], fmt)
        add(f"[P, -P, Q] fmt {fmt}", [Pk, neg(Pk), Q], fmt)
    # a refused key first, last and at a chunk boundary (the all-zero object; the x-only and compressed x = p)
    for nm, fmt, badkey in (("all-zero object", 1, bytes(64)), ("x = p", 0, b32(P)), ("compressed x = p", 2, b"\x02" + b32(P)), ("uncompressed prefix 05", 3, b"\x05" + ref.encode(pool[0], 4)),
                            ("affine y = p", 4, pool[0][31::-1] + b32(P))):
        good = [ref.encode(o, fmt) for o in pool[:2 * F]]
        for pos in ((0, 2 * F - 1, F - 1, F) if fmt <= 2 else (F,)):      # first, last and at both sides of the chunk boundary
            ks = list(good); ks[pos] = badkey
            out.append(combine_item(ref, f"refused key ({nm}) at {pos} of {2 * F}", fmt, ks))
        out.append(combine_item(ref, f"refused key ({nm}) alone", fmt, [badkey]))
    assert 0 < sum(x[3] for x in out) < len(out)
    return out


def edge_cases(ref, fanin=FANIN):
    return {"convert": convert_edges(ref), "tweak_mul": tweak_mul_edges(ref), "combine": combine_edges(ref, fanin)}


def random_items(ref, n, seed):
    """n seeded items per call; every fourth one is corrupted in one random bit of its key (never of an object: a point off the curve
    is not comparable)"""
    rng = np.random.default_rng(seed)
    keys = [ref.ec_create(_seckey(rng)) for _ in range(16)]

    def key(i, fmt):
        k = ref.encode(keys[int(rng.integers(0, len(keys)))], fmt)
        if i % 4 == 3 and fmt != 1:
            bit = int(rng.integers(0, 8 * len(k)))
            k = bytearray(k); k[bit >> 3] ^= 1 << (bit & 7); k = bytes(k)
        return k

    conv, tm, comb = [], [], []
    for i in range(n):
        fmt = int(rng.integers(0, 5))
        conv.append(convert_item(ref, f"random {i}", fmt, key(i, fmt)))
        fmt = int(rng.integers(0, 5))
        tm.append(tweak_mul_item(ref, f"random {i}", fmt, key(i, fmt), bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())))
        fmt = int(rng.integers(0, 5)); m = int(rng.integers(1, 6))
        comb.append(combine_item(ref, f"random {i}", fmt, [key(i if j == m - 1 else 0, fmt) for j in range(m)]))
    return {"convert": conv, "tweak_mul": tm, "combine": comb}


def derive_outs(obj64):
    """an object (None: refused) -> (the six output encodings, parity), by byte shuffling and one subtraction: what the recorded file
    does not store.  The tests hold it against the reference's own serialisers (edge_cases() == the recorded list)."""
    if obj64 is None:
        return tuple(bytes(PK_BYTES[f]) for f in OUT_FORMATS), 0
    x, y = obj64[31::-1], obj64[:31:-1]
    par = y[31] & 1
    even = y if not par else b32(P - int.from_bytes(y, "big"))
    return (x, bytes(obj64), bytes([2 + par]) + x, b"\x04" + x + y, x + y, obj64[:32] + even[::-1]), par


def negated(obj64):
    return None if obj64 is None else obj64[:32] + b32(P - int.from_bytes(obj64[:31:-1], "big"))[::-1]


def to_json(items):
    """{call: items} -> {"blobs": every distinct key, tweak and result object once, as hex; call: rows that name them by index}.  A row
    keeps the name, the format, the key(s), the tweak, the verdict and the result OBJECT (null: refused); the other encodings, the parity
    and the negation are derive_outs() / negated() of it."""
    blobs, index = [], {}

    def ref_(b):
        b = bytes(b)
        if b not in index:
            index[b] = len(blobs); blobs.append(b.hex())
        return index[b]
    out = {"convert": [[n, f, ref_(k), v, ref_(o[1]) if v else None] for n, f, k, v, o, p, no, np_ in items["convert"]],
           "tweak_mul": [[n, f, ref_(k), ref_(t), v, ref_(o[1]) if v else None] for n, f, k, t, v, o, p in items["tweak_mul"]],
           "combine": [[n, f, [ref_(k) for k in ks], v, ref_(o[1]) if v else None] for n, f, ks, v, o, p in items["combine"]]}
    out["blobs"] = blobs
    return out


def from_json(d):
    B = [bytes.fromhex(h) for line in d["blobs"] for h in line.split()]      # (eight to a line in the file)
    obj = lambda i: None if i is None else B[i]      # noqa: E731
    conv = [(n, f, B[k], v) + derive_outs(obj(o)) + derive_outs(negated(obj(o))) for n, f, k, v, o in d["convert"]]
    tm = [(n, f, B[k], B[t], v) + derive_outs(obj(o)) for n, f, k, t, v, o in d["tweak_mul"]]
    comb = [(n, f, [B[k] for k in ks], v) + derive_outs(obj(o)) for n, f, ks, v, o in d["combine"]]
    return {"convert": conv, "tweak_mul": tm, "combine": comb}
