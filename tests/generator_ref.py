"""ctypes view of the reference's generator module in oracle/_ref/libsecp256k1_ref.so (include/secp256k1_generator.h), the edge list
the generator tests share, and a plain-Python restatement of the Shallue-van de Woestijne map and of generate on top of it.  Test-only.

The reference keeps the map `static`, so the Python model is the yardstick of the lane-level cases (a chosen t, a chosen (t1, t2));
tests/test_cpu_generator.py first holds the model's generate against secp256k1_generator_generate[_blinded] on 576 keys.

An item is the tuple  (op, name, args, verdict, out)
    op "parse":     args (in33,)                         out: the 64-byte generator object, zeros where verdict == 0
    op "serialize": args (gen64,)                        out: 33 bytes; verdict 1
    op "generate":  args (key32, blind32 or None)        out: the 64-byte object, zeros where verdict == 0 (the engine's contract: the
                                                         reference writes a generator from the reduced blind and returns 0)
    op "commit":    args (blind32 or None, value, gen64) out: 33 bytes (9 ^ is_square(y) | x), zeros where verdict == 0
Every verdict and every output of a verdict-1 item is the reference's, asked when the list is built; the one exception is the commit items
on malformed generator objects (all zero, y = 0), which are the engine's contract alone: 0 and zero bytes."""
import ctypes
import hashlib

import numpy as np

from tests.refapi import REF_PATH, N, P, G_XY, GENERATOR_H  # noqa: F401

CONTEXT_NONE = 1
EC_UNCOMPRESSED = 1 << 1
_vp, _int = ctypes.c_void_p, ctypes.c_int


class GeneratorRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_generator_parse": [_vp, _vp, _vp],
            "secp256k1_generator_serialize": [_vp, _vp, _vp],
            "secp256k1_generator_generate": [_vp, _vp, _vp],
            "secp256k1_generator_generate_blinded": [_vp, _vp, _vp, _vp],
            "secp256k1_pedersen_commit": [_vp, _vp, _vp, ctypes.c_uint64, _vp],
            "secp256k1_pedersen_commitment_serialize": [_vp, _vp, _vp],
            "secp256k1_pedersen_verify_tally": [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t],
            "secp256k1_ec_pubkey_create": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_serialize": [_vp, _vp, _vp, _vp, ctypes.c_uint],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx
        self.generator_h = ctypes.string_at(ctypes.c_void_p.in_dll(L, "secp256k1_generator_h").value, 64)

    def parse(self, in33):
        o = ctypes.create_string_buffer(64)
        return (1, o.raw) if self.lib.secp256k1_generator_parse(self.ctx, o, bytes(in33)) == 1 else (0, bytes(64))

    def serialize(self, gen64):
        o = ctypes.create_string_buffer(33)
        assert self.lib.secp256k1_generator_serialize(self.ctx, o, bytes(gen64)) == 1
        return o.raw

    def generate_raw(self, key32, blind32=None):
        """(the reference's return value, what it wrote)"""
        o = ctypes.create_string_buffer(64)
        if blind32 is None:
            r = self.lib.secp256k1_generator_generate(self.ctx, o, bytes(key32))
        else:
            r = self.lib.secp256k1_generator_generate_blinded(self.ctx, o, bytes(key32), bytes(blind32))
        return r, o.raw

    def generate(self, key32, blind32=None):
        r, o = self.generate_raw(key32, blind32)
        return (1, o) if r == 1 else (0, bytes(64))

    def commit_obj(self, blind32, value, gen64):
        """-> the 64-byte commitment object, or None"""
        o = ctypes.create_string_buffer(64)
        r = self.lib.secp256k1_pedersen_commit(self.ctx, o, bytes(32) if blind32 is None else bytes(blind32), int(value), bytes(gen64))
        return o.raw if r == 1 else None

    def commit(self, blind32, value, gen64):
        """(verdict, 33 bytes): NULL blinds of the engine are the all-zero blind of the reference"""
        obj = self.commit_obj(blind32, value, gen64)
        if obj is None:
            return 0, bytes(33)
        o = ctypes.create_string_buffer(33)
        assert self.lib.secp256k1_pedersen_commitment_serialize(self.ctx, o, obj) == 1 and o.raw == obj[:33]
        return 1, o.raw

    def verify_tally(self, pos_objs, neg_objs):
        def arr(objs):
            bufs = [ctypes.create_string_buffer(bytes(o), 64) for o in objs]
            ptrs = (ctypes.c_void_p * max(len(bufs), 1))(*[ctypes.addressof(b) for b in bufs])
            return bufs, ptrs
        pb, pp = arr(pos_objs); nb, np_ = arr(neg_objs)
        return self.lib.secp256k1_pedersen_verify_tally(self.ctx, pp, len(pos_objs), np_, len(neg_objs))

    def gen_from_seckey(self, k):
        """k*G as a generator object (x | y big-endian), through secp256k1_ec_pubkey_create and the uncompressed serialisation"""
        pk = ctypes.create_string_buffer(64); ser = ctypes.create_string_buffer(65); ln = ctypes.c_size_t(65)
        assert self.lib.secp256k1_ec_pubkey_create(self.ctx, pk, b32(k)) == 1
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, ser, ctypes.byref(ln), pk, EC_UNCOMPRESSED) == 1 and ser.raw[0] == 4
        return ser.raw[1:]


def b32(v):
    return int(v).to_bytes(32, "big")


# ---- the plain-Python model ----------------------------------------------------------------------------------------------------------
NEGC = 0xf5d2d456caf80e20dcc88f3d586869d339e092ea25eb132b8272d850e32a03dd      # -sqrt(-3)
D = 0x851695d49a83f8ef919bb86153cbcb16630fb68aed0a766a3ec693d68e6afa40         # (sqrt(-3) - 1) / 2
assert NEGC * NEGC % P == P - 3 and (2 * D + 1 + NEGC) % P == 0
GX, GY = int.from_bytes(G_XY[:32], "big"), int.from_bytes(G_XY[32:], "big")


def model_map(t):
    """shallue_van_de_woestijne(t), 0 <= t < p -> (x, y, branch): branch 0, 1, 2 for the candidates x1, x2, x3"""
    t2 = t * t % P
    wd = (8 + t2) % P
    x3d = -3 * t2 % P
    j = wd * x3d % P
    jinv = pow(j, P - 2, P)                                         # 0 for j == 0, as secp256k1_fe_inv
    x1 = (D + NEGC * t2 * x3d * jinv) % P
    x2 = -(x1 + 1) % P
    x3 = (1 + wd * wd * wd * jinv) % P
    roots = []
    for x in (x1, x2, x3):
        a = (x * x * x + 7) % P
        y = pow(a, (P + 1) // 4, P)                                 # the root secp256k1_fe_sqrt returns
        roots.append((x, y, y * y % P == a))
    branch = 0 if roots[0][2] else (1 if roots[1][2] else 2)
    x, y, _ = roots[branch]
    if t & 1:
        y = -y % P
    return x, y, branch


def _padd(a, b):
    """affine addition; None is infinity"""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def _pmul(k, a):
    r = None
    while k:
        if k & 1:
            r = _padd(r, a)
        a = _padd(a, a); k >>= 1
    return r


def model_hash_t(key32):
    return tuple(int.from_bytes(hashlib.sha256(pfx + bytes(key32)).digest(), "big") for pfx in (b"1st generation: ", b"2nd generation: "))


def model_from_t(t1, t2, blind=None):
    """(verdict, 64 bytes, (branch1, branch2)): [blind*G +] map(t1) + map(t2); infinity gives verdict 0 and zeros (the engine's contract)"""
    x1, y1, b1 = model_map(t1); x2, y2, b2 = model_map(t2)
    acc = None if blind is None else _pmul(blind % N, (GX, GY))
    acc = _padd(_padd(acc, (x1, y1)), (x2, y2))
    ok = acc is not None and (blind is None or blind < N)
    return (1, b32(acc[0]) + b32(acc[1]), (b1, b2)) if ok else (0, bytes(64), (b1, b2))


def model_generate(key32, blind32=None):
    t1, t2 = model_hash_t(key32)
    assert t1 < P and t2 < P
    return model_from_t(t1, t2, None if blind32 is None else int.from_bytes(blind32, "big"))


# ---- the edge list ----------------------------------------------------------------------------------------------------------------
def _rand32(rng):
    return bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())


def _item(ref, op, name, *args):
    if op == "parse":
        v, out = ref.parse(*args)
    elif op == "serialize":
        v, out = 1, ref.serialize(*args)
    elif op == "generate":
        v, out = ref.generate(*args)
    else:
        v, out = ref.commit(*args)
    return (op, name, tuple(args), v, out)


def edge_cases(ref):
    rng = np.random.default_rng(5501)
    out = []

    def add(op, name, *args):
        out.append(_item(ref, op, name, *args))

    # parse: both prefixes on a valid x, refused prefixes, x values, an x off the curve
    hx = ref.generator_h[:32]
    for pfx in (0x0a, 0x0b):
        add("parse", f"prefix {pfx:02x} valid x", bytes([pfx]) + hx)
    for pfx in (0x00, 0x02, 0x08, 0x09, 0x0c, 0xff):
        add("parse", f"prefix {pfx:02x} refused", bytes([pfx]) + hx)
    for nm, x in (("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^256-1", (1 << 256) - 1)):
        for pfx in (0x0a, 0x0b):
            add("parse", f"x = {nm} prefix {pfx:02x}", bytes([pfx]) + b32(x))
    x_off = next(x for x in range(2, 100) if ref.parse(b"\x0a" + b32(x))[0] == 0)
    add("parse", f"x = {x_off} not on the curve", b"\x0a" + b32(x_off))
    for i in range(4):
        g = ref.generate(_rand32(rng))[1]
        add("parse", f"generated x {i}", bytes([0x0a + (i & 1)]) + g[:32])
    # serialize: the generators parse accepted, secp256k1_generator_h; parse of serialize is the identity
    accepted = [it[4] for it in out if it[0] == "parse" and it[3] == 1]
    for i, g in enumerate(accepted):
        add("serialize", f"accepted {i}", g)
    add("serialize", "generator_h", ref.generator_h)
    for it in [x for x in out if x[0] == "serialize"]:
        assert ref.parse(it[4]) == (1, it[2][0]), it[1]
    assert {it[4][0] for it in out if it[0] == "serialize"} == {0x0a, 0x0b}
    # generate: plain, and blinds around n
    key = _rand32(rng)
    add("generate", "plain", key, None)
    add("generate", "key all zero", bytes(32), None)
    add("generate", "key all ones", b"\xff" * 32, None)
    for nm, v in (("0", 0), ("1", 1), ("n-1", N - 1), ("n", N), ("n+1", N + 1), ("2^256-1", (1 << 256) - 1)):
        add("generate", f"blind {nm}", key, b32(v))
    add("generate", "blind random", key, _rand32(rng))
    assert [it[3] for it in out if it[1].startswith("blind ")] == [1, 1, 1, 0, 0, 0, 1]
    assert next(it[4] for it in out if it[1] == "blind 0") == next(it[4] for it in out if it[1] == "plain")        # blind 0 is the plain generator
    # commit
    k = int.from_bytes(_rand32(rng), "big") % N
    gk = ref.gen_from_seckey(k)
    gens = (("kG", gk), ("generated", ref.generate(key)[1]), ("generator_h", ref.generator_h))
    blinds = (("0", 0), ("1", 1), ("n-1", N - 1), ("n", N), ("2^256-1", (1 << 256) - 1))
    values = (("0", 0), ("1", 1), ("2^63", 1 << 63), ("2^64-1", (1 << 64) - 1))
    for gn, g in gens:
        for vn, v in values:
            add("commit", f"{gn} value {vn} NULL blinds", None, v, g)
            for bn, b in blinds:
                add("commit", f"{gn} value {vn} blind {bn}", b32(b), v, g)
    for vn, v in values[1:] + (("random", int(rng.integers(1, 1 << 62))),):
        add("commit", f"kG value {vn} blind n - value k: infinity", b32((N - v * k) % N), v, gk)
        add("commit", f"kG value {vn} blind value k: doubling", b32(v * k % N), v, gk)
    # malformed objects (engine only: the reference is not asked -- it reads an off-curve point unchecked): the all-zero object, which parse
    # and generate write for a refused item, and an object with y = 0 are refused whatever value and blind are
    for gn, g in (("all-zero object", bytes(64)), ("object with y = 0", b32(5) + bytes(32))):
        for vn, v in (("0", 0), ("1", 1), ("7", 7), ("2^63", 1 << 63)):
            for bn, b in (("NULL blinds", None), ("blind 1", b32(1))):
                out.append(("commit", f"{gn} value {vn} {bn}", (b, v, g), 0, bytes(33)))
    names = {it[1]: it for it in out}
    assert all(it[3] == 0 for it in out if "infinity" in it[1]) and all(it[3] == 1 for it in out if "doubling" in it[1])
    assert names["kG value 0 NULL blinds"][3] == 0 and names["kG value 0 blind 0"][3] == 0 and names["kG value 1 blind n"][3] == 0
    assert names["kG value 1 NULL blinds"][4] == names["kG value 1 blind 0"][4] and names["kG value 1 NULL blinds"][3] == 1
    return out


def random_items(ref, n, seed):
    """n seeded items per entry point: parse (every fourth one a random x with a random prefix byte), serialize, generate (every other one
    blinded, every eighth one with a blind >= n), commit (every third one with NULL blinds, every eighth one with a blind >= n)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        g = ref.generate(_rand32(rng))[1]
        ser = ref.serialize(g)
        if i % 4 == 3:
            ser = bytes([int(rng.integers(0, 256)) if i % 8 == 7 else 0x0a]) + _rand32(rng)
        out.append(_item(ref, "parse", f"random parse {i}", ser))
        out.append(_item(ref, "serialize", f"random serialize {i}", g))
        big = b32(int(rng.integers(0, 1 << 60)) + N)
        blind = None if i % 2 == 0 else (big if i % 8 == 7 else _rand32(rng))
        out.append(_item(ref, "generate", f"random generate {i}", _rand32(rng), blind))
        blind = None if i % 3 == 0 else (big if i % 8 == 7 else _rand32(rng))
        out.append(_item(ref, "commit", f"random commit {i}", blind, int(rng.integers(0, 1 << 64, dtype=np.uint64)), g))
    return out


def _hex(v):
    return v.hex() if isinstance(v, (bytes, bytearray)) else v


def to_json(items):
    return [[op, nm, [_hex(a) for a in args], v, out.hex()] for op, nm, args, v, out in items]


def from_json(rows):
    return [(op, nm, tuple(bytes.fromhex(a) if isinstance(a, str) else a for a in args), v, bytes.fromhex(out)) for op, nm, args, v, out in rows]
