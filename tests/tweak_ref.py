"""ctypes view of the reference's public key-tweak API in oracle/_ref/libsecp256k1_ref.so (include/secp256k1.h,
include/secp256k1_extrakeys.h) and the edge list the tweak tests share.  Test-only.  Every expected verdict and output key is the
reference's own, asked when the list is built; the one exception is the all-zero key object (engine only, verdict 0: there the
reference calls its illegal-argument callback).

An item is the tuple
    (name, key_format, key, tweak32, tweaked32, parity, check_verdict, add_verdict, out64)
key_format 0: 32-byte x-only key, 1: 64-byte key object, 2: 33-byte compressed key.  tweaked32 / parity are the check form's inputs;
check_verdict is None for key_format 2 (the check form does not take it).  add_verdict / out64 are None where the add form's output is
not comparable: a key OBJECT with a flipped bit is a point off the curve, which neither side refuses and on which two correct
implementations of the group law need not agree (the check form's verdict, 0, is still compared)."""
import ctypes

import numpy as np

from tests.refapi import REF_PATH, N, P  # noqa: F401

CONTEXT_NONE = 1
EC_COMPRESSED = (1 << 1) | (1 << 8)

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class TweakRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_xonly_pubkey_parse": [_vp, _vp, _vp],
            "secp256k1_xonly_pubkey_tweak_add": [_vp, _vp, _vp, _vp],
            "secp256k1_xonly_pubkey_tweak_add_check": [_vp, _vp, _int, _vp, _vp],
            "secp256k1_xonly_pubkey_from_pubkey": [_vp, _vp, _vp, _vp],
            "secp256k1_ec_pubkey_parse": [_vp, _vp, _vp, _sz],
            "secp256k1_ec_pubkey_create": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_negate": [_vp, _vp],
            "secp256k1_ec_pubkey_tweak_add": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_serialize": [_vp, _vp, _vp, _vp, ctypes.c_uint],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx

    # ---- the nine calls; key objects are 64 bytes ----------------------------------------------------------------------------------------
    def xonly_parse(self, x32):
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_xonly_pubkey_parse(self.ctx, o, bytes(x32)) == 1 else None

    def xonly_tweak_add(self, xobj64, tweak32):
        """-> the secp256k1_pubkey object, or None"""
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_xonly_pubkey_tweak_add(self.ctx, o, bytes(xobj64), bytes(tweak32)) == 1 else None

    def xonly_tweak_add_check(self, tweaked32, parity, xobj64, tweak32):
        return self.lib.secp256k1_xonly_pubkey_tweak_add_check(self.ctx, bytes(tweaked32), int(parity), bytes(xobj64), bytes(tweak32))

    def xonly_from_pubkey(self, obj64):
        o = ctypes.create_string_buffer(64); par = _int(-1)
        assert self.lib.secp256k1_xonly_pubkey_from_pubkey(self.ctx, o, ctypes.byref(par), bytes(obj64)) == 1
        return o.raw, par.value

    def ec_parse(self, ser):
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ec_pubkey_parse(self.ctx, o, bytes(ser), len(ser)) == 1 else None

    def ec_create(self, seckey32):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ec_pubkey_create(self.ctx, o, bytes(seckey32)) == 1
        return o.raw

    def ec_negate(self, obj64):
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        assert self.lib.secp256k1_ec_pubkey_negate(self.ctx, o) == 1
        return o.raw

    def ec_tweak_add(self, obj64, tweak32):
        """-> the tweaked object, or None (the reference zeroes the object then)"""
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        if self.lib.secp256k1_ec_pubkey_tweak_add(self.ctx, o, bytes(tweak32)) == 1:
            return o.raw
        assert o.raw == bytes(64)
        return None

    def ec_serialize(self, obj64):
        o = ctypes.create_string_buffer(33); ln = _sz(33)
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, o, ctypes.byref(ln), bytes(obj64), EC_COMPRESSED) == 1
        return o.raw

    # ---- what the engine's two batch forms are compared with ----------------------------------------------------------------------------
    def check(self, key_format, key, tweaked32, parity, tweak32):
        """results[i] of the check form: key_format 0 parses first"""
        obj = self.xonly_parse(key) if key_format == 0 else bytes(key)
        return 0 if obj is None else self.xonly_tweak_add_check(tweaked32, parity, obj, tweak32)

    def add(self, key_format, key, tweak32):
        """(results[i], pubkeys_out64[i]) of the add form"""
        if key_format == 2:
            obj = self.ec_parse(key)
            out = None if obj is None else self.ec_tweak_add(obj, tweak32)
        else:
            obj = self.xonly_parse(key) if key_format == 0 else bytes(key)
            out = None if obj is None else self.xonly_tweak_add(obj, tweak32)
            if key_format == 1:
                assert out == self.ec_tweak_add(obj, tweak32)          # the two reference functions share their core
        return (0, bytes(64)) if out is None else (1, out)


def obj_x32(obj64):
    """key object -> its x, 32 big-endian bytes (the serialised x-only key)"""
    return bytes(obj64[31::-1])


def obj_parity(obj64):
    return obj64[32] & 1


def b32(v):
    return int(v).to_bytes(32, "big")


def _flip(b, bit):
    b = bytearray(b); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)


def _seckey(rng):
    return bytes(rng.integers(0, 256, 31, dtype=np.uint8).tolist()) + b"\x01"


TABLE_WIDTHS = (12, 20, 26)          # the host emulation's generator table, the device's two


def boundary_tweaks():
    """-> list of (D, w, tweak int): the six values around window w's lowest bit and around its sign threshold, for every table width"""
    out = []
    for D in TABLE_WIDTHS:
        for w in (1, 2, -(-256 // D) - 1):
            for base in (D * w, D * w - 1):
                for d in (-1, 0, 1):
                    out.append((D, w, (1 << base) + d))
    return out


def make_item(ref, name, key_format, key, tweak32, tweaked32=None, parity=None, add=True, engine_only=False):
    """tweaked32 / parity default to what the reference's add form gives (a valid check), or zeros where it gives nothing"""
    key, tweak32 = bytes(key), bytes(tweak32)
    if engine_only:
        av, out = 0, bytes(64)
    else:
        av, out = ref.add(key_format, key, tweak32) if add else (None, None)
    if tweaked32 is None:
        tweaked32 = obj_x32(out) if av else bytes(32)
    if parity is None:
        parity = obj_parity(out) if av else 0
    cv = None if key_format == 2 else (0 if engine_only else ref.check(key_format, key, tweaked32, parity, tweak32))
    return (name, key_format, key, tweak32, bytes(tweaked32), int(parity), cv, av, out)


def edge_cases(ref):
    rng = np.random.default_rng(4401)
    out = []

    def add(*a, **k):
        out.append(make_item(ref, *a, **k))

    # valid checks of both parities, in both key formats, then the same items mutated
    keys = [ref.ec_create(_seckey(rng)) for _ in range(4)]
    seen = set()
    for i in range(64):
        obj = keys[i % 4]; t = _seckey(rng)
        xobj, _ = ref.xonly_from_pubkey(obj)
        _, res = ref.add(1, xobj, t)
        par = obj_parity(res)
        if par in seen:
            continue
        seen.add(par)
        for fmt, key in ((0, obj_x32(obj)), (1, xobj)):
            _, res = ref.add(fmt, key, t)
            tw, pr = obj_x32(res), obj_parity(res)
            base = f"parity {par} fmt {fmt}"
            add("valid " + base, fmt, key, t)
            add(base + ": parity ^ 1", fmt, key, t, tw, pr ^ 1)
            add(base + ": parity byte 2", fmt, key, t, tw, 2)
            add(base + ": parity byte 255", fmt, key, t, tw, 255)
            add(base + ": tweaked32 bit flipped", fmt, key, t, _flip(tw, 8 * 13 + 2), pr)
            add(base + ": tweak bit flipped", fmt, key, _flip(t, 8 * 20 + 5), tw, pr)
            # (a flipped bit in an x-only key gives another key or none; in an object it gives a point off the curve: check form only)
            add(base + ": key bit flipped", fmt, _flip(key, 8 * 9 + 1), t, tw, pr, add=(fmt == 0))
        if len(seen) == 2:
            break
    assert seen == {0, 1}
    # tweak values
    obj = keys[0]; xobj, _ = ref.xonly_from_pubkey(obj)
    for nm, v in (("0", 0), ("1", 1), ("n-1", N - 1), ("n", N), ("n+1", N + 1), ("2^256-1", (1 << 256) - 1)):
        add(f"tweak {nm} fmt 0", 0, obj_x32(obj), b32(v))
        add(f"tweak {nm} fmt 1", 1, xobj, b32(v))
        add(f"tweak {nm} fmt 2", 2, ref.ec_serialize(obj), b32(v))
    # a key with a known secret key: infinity and the doubling, on P and on -P
    k = int.from_bytes(_seckey(rng), "big") % N
    Pk = ref.ec_create(b32(k))
    for nm, Q in (("P", Pk), ("-P", ref.ec_negate(Pk))):
        for tn, t in (("n-k", N - k), ("k", k)):
            add(f"{nm} = kG, t = {tn}, fmt 1", 1, Q, b32(t))
            add(f"{nm} = kG, t = {tn}, fmt 0", 0, obj_x32(Q), b32(t))
            add(f"{nm} = kG, t = {tn}, fmt 2", 2, ref.ec_serialize(Q), b32(t))
    # boundaries of the fixed-base recoding: on an ordinary key, and on the window's own base point and its negation, so that the final
    # addition meets a table record itself
    for D, w, t in boundary_tweaks():
        add(f"recoding D={D} w={w} t={t:#x}", 1, keys[1], b32(t))
    for D in TABLE_WIDTHS:
        for w in (1, 2, -(-256 // D) - 1):
            B = ref.ec_create(b32(1 << (D * w)))
            for nm, Q in (("B", B), ("-B", ref.ec_negate(B))):
                for d in (-1, 0, 1):
                    for base in (D * w, D * w - 1):
                        t = (1 << base) + d
                        add(f"recoding D={D} w={w} t={t:#x} on {nm}", 1, Q, b32(t))
    # format 0 keys
    t = _seckey(rng)
    x_off = next(x for x in range(2, 100) if ref.xonly_parse(b32(x)) is None)
    for nm, x in (("x = p", P), ("x = p + 1", P + 1), ("x = 2^256 - 1", (1 << 256) - 1), ("x = p - 1", P - 1), (f"x = {x_off} not on the curve", x_off), ("x = 0", 0)):
        add("fmt 0 " + nm, 0, b32(x), t)
    # format 1 keys: a secp256k1_pubkey with odd y handed in as it is, and the all-zero object
    odd = next(o for o in (ref.ec_create(_seckey(rng)) for _ in range(64)) if obj_parity(o) == 1)
    add("fmt 1 object with odd y", 1, odd, t)
    add("fmt 1 object with odd y, t = 0", 1, odd, b32(0))
    add("fmt 1 all-zero object", 1, bytes(64), t, engine_only=True)
    # format 2 keys
    for j, Q in enumerate(keys[:3] + [odd]):
        ser = ref.ec_serialize(Q)
        add(f"fmt 2 key {j} prefix {ser[0]:02x}", 2, ser, t)
    ser = ref.ec_serialize(keys[0])
    for pfx in (0x00, 0x04, 0x05, 0x06):
        add(f"fmt 2 bad prefix {pfx:02x}", 2, bytes([pfx]) + ser[1:], t)
    add("fmt 2 x not on the curve", 2, b"\x02" + b32(x_off), t)
    add("fmt 2 x = p", 2, b"\x03" + b32(P), t)
    prefixes = {it[2][0] for it in out if it[1] == 2 and it[7] == 1}
    assert prefixes == {2, 3}
    return out


def random_items(ref, n, seed):
    """seeded items on valid keys with distinct random tweaks, the two key formats alternating; every fourth one is corrupted in one random bit of one
    of its inputs (tweaked32, parity byte, tweak, or -- x-only keys only -- the key)"""
    rng = np.random.default_rng(seed)
    keys = [ref.ec_create(_seckey(rng)) for _ in range(8)]
    out = []
    for i in range(n):
        obj = keys[int(rng.integers(0, len(keys)))]; fmt = (i + i // 4) % 2      # (both formats among the corrupted items, i % 4 == 3)
        key = obj_x32(obj) if fmt == 0 else ref.xonly_from_pubkey(obj)[0]
        t = bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())
        _, res = ref.add(fmt, key, t)
        tw, par = obj_x32(res), obj_parity(res)
        if i % 4 == 3:
            which = int(rng.integers(0, 4 if fmt == 0 else 3))
            if which == 0:
                tw = _flip(tw, int(rng.integers(0, 256)))
            elif which == 1:
                par ^= 1 << int(rng.integers(0, 8))
            elif which == 2:
                t = _flip(t, int(rng.integers(0, 256)))
            else:
                key = _flip(key, int(rng.integers(0, 256)))
        out.append(make_item(ref, f"random {i}", fmt, key, t, tw, par))
    return out


def to_json(items):
    return [[nm, fmt, key.hex(), t.hex(), tw.hex(), par, cv, av, None if o is None else o.hex()] for nm, fmt, key, t, tw, par, cv, av, o in items]


def from_json(rows):
    return [(nm, fmt, bytes.fromhex(key), bytes.fromhex(t), bytes.fromhex(tw), par, cv, av, None if o is None else bytes.fromhex(o))
            for nm, fmt, key, t, tw, par, cv, av, o in rows]
