"""ctypes view of the reference's public whitelist API in oracle/_ref/libsecp256k1_ref.so (include/secp256k1_whitelist.h) and the
edge list the whitelist tests share.  Test-only.  Every expected verdict is the reference's own, asked when the list is built."""
import ctypes
import hashlib

import numpy as np

from tests.refapi import REF_PATH, N  # noqa: F401

CONTEXT_NONE = 1
EC_COMPRESSED = (1 << 1) | (1 << 8)

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class WhitelistSignature(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_size_t), ("data", ctypes.c_ubyte * (32 * 256))]


class WhitelistRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_whitelist_sign": [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz],
            "secp256k1_whitelist_verify": [_vp, _vp, _vp, _vp, _sz, _vp],
            "secp256k1_whitelist_signature_parse": [_vp, _vp, _vp, _sz],
            "secp256k1_whitelist_signature_serialize": [_vp, _vp, _vp, _vp],
            "secp256k1_ec_pubkey_create": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_negate": [_vp, _vp],
            "secp256k1_ec_pubkey_combine": [_vp, _vp, _vp, _sz],
            "secp256k1_ec_pubkey_tweak_mul": [_vp, _vp, _vp],
            "secp256k1_ec_seckey_tweak_add": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_serialize": [_vp, _vp, _vp, _vp, ctypes.c_uint],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx

    # ---- keys (64-byte secp256k1_pubkey objects as bytes) ------------------------------------------------------------------------------
    def pubkey_create(self, seckey32):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ec_pubkey_create(self.ctx, o, bytes(seckey32)) == 1
        return o.raw

    def pubkey_negate(self, obj64):
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        assert self.lib.secp256k1_ec_pubkey_negate(self.ctx, o) == 1
        return o.raw

    def pubkey_combine(self, objs):
        """-> the sum, or None when it is the point at infinity"""
        bufs = [ctypes.create_string_buffer(bytes(x), 64) for x in objs]
        ptrs = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ec_pubkey_combine(self.ctx, o, ptrs, len(bufs)) == 1 else None

    def pubkey_tweak_mul(self, obj64, tweak32):
        o = ctypes.create_string_buffer(bytes(obj64), 64)
        assert self.lib.secp256k1_ec_pubkey_tweak_mul(self.ctx, o, bytes(tweak32)) == 1
        return o.raw

    def seckey_tweak_add(self, seckey32, tweak32):
        o = ctypes.create_string_buffer(bytes(seckey32), 32)
        assert self.lib.secp256k1_ec_seckey_tweak_add(self.ctx, o, bytes(tweak32)) == 1
        return o.raw

    def pubkey_serialize(self, obj64):
        o = ctypes.create_string_buffer(33); ln = _sz(33)
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, o, ctypes.byref(ln), bytes(obj64), EC_COMPRESSED) == 1
        return o.raw

    # ---- signatures ------------------------------------------------------------------------------------------------------------------------
    def sign(self, online, offline, sub64, online_seckey, summed_seckey, index):
        """online / offline: lists of key objects -> the serialised signature (secp256k1_whitelist_sign + _signature_serialize)"""
        sig = WhitelistSignature()
        assert self.lib.secp256k1_whitelist_sign(self.ctx, ctypes.byref(sig), b"".join(online), b"".join(offline), len(online), bytes(sub64),
                                                 bytes(online_seckey), bytes(summed_seckey), index) == 1
        o = ctypes.create_string_buffer(33 + 32 * 256); ln = _sz(len(o))
        assert self.lib.secp256k1_whitelist_signature_serialize(self.ctx, o, ctypes.byref(ln), ctypes.byref(sig)) == 1
        return o.raw[:ln.value]

    def parse(self, ser):
        """-> WhitelistSignature or None"""
        sig = WhitelistSignature()
        buf = bytes(ser) if len(ser) else b"\0"
        return sig if self.lib.secp256k1_whitelist_signature_parse(self.ctx, ctypes.byref(sig), buf, len(ser)) == 1 else None

    def verify(self, ser, online, offline, sub64):
        """secp256k1_whitelist_signature_parse && secp256k1_whitelist_verify; online / offline: bytes, 64 per key (equal lengths)"""
        sig = self.parse(ser)
        if sig is None:
            return 0
        n = len(online) // 64
        pad = b"\0" * 64                                              # (n == 0: the reference's ARG_CHECK still wants non-NULL arrays)
        return self.lib.secp256k1_whitelist_verify(self.ctx, ctypes.byref(sig), bytes(online) + pad, bytes(offline) + pad, n, bytes(sub64))


def _seckey(rng):
    return bytes(rng.integers(0, 256, 31, dtype=np.uint8).tolist()) + b"\x01"


class Whitelist:
    """n key pairs made once: secret and public halves"""
    def __init__(self, ref, rng, n):
        self.on_sec = [_seckey(rng) for _ in range(n)]; self.off_sec = [_seckey(rng) for _ in range(n)]
        self.online = [ref.pubkey_create(k) for k in self.on_sec]; self.offline = [ref.pubkey_create(k) for k in self.off_sec]
        self.n = n

    def sign(self, ref, rng, index, online=None, offline=None):
        """a fresh sub key and a signature by key `index` -> (sig, sub64); online / offline override the PUBLIC lists that are signed over"""
        sub_sec = _seckey(rng); sub = ref.pubkey_create(sub_sec)
        summed = ref.seckey_tweak_add(self.off_sec[index], sub_sec)
        return ref.sign(online or self.online, offline or self.offline, sub, self.on_sec[index], summed, index), sub


def crafted_empty(ref, sub64):
    """the 0-key signature the reference accepts: e0 = SHA256(msg32), msg32 = SHA256(ser33(sub))"""
    return b"\0" + hashlib.sha256(hashlib.sha256(ref.pubkey_serialize(sub64)).digest()).digest()


def ring_key(ref, online64, offline64, sub64):
    """K = online + t (offline + sub) from the reference's public calls -> key object, or None for infinity"""
    a = ref.pubkey_combine([offline64, sub64])
    if a is None:
        return online64
    t = hashlib.sha256(ref.pubkey_serialize(a)).digest()
    return ref.pubkey_combine([ref.pubkey_tweak_mul(a, t), online64])


def _flip(b, bit):
    b = bytearray(b); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)


def edge_cases(ref, with_255=False):
    """-> list of (name, sig, online bytes, offline bytes, sub64, expected).  expected is the reference's verdict, except for the
    all-zero key object (engine only, 0: there the reference calls its illegal-argument callback and reads an unset point)."""
    rng = np.random.default_rng(3301)
    out = []

    def add(name, sig, online, offline, sub, engine_only=None):
        online, offline = b"".join(online), b"".join(offline)
        out.append((name, bytes(sig), online, offline, bytes(sub), ref.verify(sig, online, offline, sub) if engine_only is None else engine_only))

    lists = {n: Whitelist(ref, rng, n) for n in (1, 2, 3, 15)}
    for n, signers in ((1, (0,)), (2, (0, 1)), (3, (0, 1, 2)), (15, (0, 7, 14))):
        for idx in signers:
            sig, sub = lists[n].sign(ref, rng, idx)
            add(f"valid n={n} signer={idx}", sig, lists[n].online, lists[n].offline, sub)
    # the empty ring
    sub0 = ref.pubkey_create(_seckey(rng))
    add("crafted n=0", crafted_empty(ref, sub0), [], [], sub0)
    add("crafted n=0, e0 bit flipped", _flip(crafted_empty(ref, sub0), 8 + 77), [], [], sub0)
    # mutations of one 3-key signature (signer 1)
    w = lists[3]; on, off = w.online, w.offline
    sig, sub = w.sign(ref, rng, 1)
    add("base n=3", sig, on, off, sub)
    add("e0 bit flipped", _flip(sig, 8 * 1 + 5), on, off, sub)
    for j, nm in ((0, "first"), (1, "middle"), (2, "last")):
        add(f"{nm} s bit flipped", _flip(sig, 8 * (33 + 32 * j) + 9), on, off, sub)
    add("sub bit flipped", sig, on, off, _flip(sub, 3))
    add("online key bit flipped", sig, [on[0], _flip(on[1], 10), on[2]], off, sub)
    add("offline key bit flipped", sig, on, [off[0], off[1], _flip(off[2], 300)], sub)
    for nm, v in (("0", 0), ("n", N), ("n+1", N + 1)):
        for j in (0, 2):
            add(f"s_{j} = {nm}", sig[:33 + 32 * j] + v.to_bytes(32, "big") + sig[65 + 32 * j:], on, off, sub)
    add("n_keys byte one too small", bytes([2]) + sig[1:], on, off, sub)
    add("n_keys byte one too large", bytes([4]) + sig[1:], on, off, sub)
    add("one byte short", sig[:-1], on, off, sub)
    add("one byte long", sig + b"\x01", on, off, sub)
    add("length 0", b"", on, off, sub)
    add("one s short, n_keys byte adjusted", bytes([2]) + sig[1:-32], on, off, sub)      # parses as a 2-key signature against a 3-key list
    add("lists swapped", sig, off, on, sub)
    add("two keys exchanged", sig, [on[1], on[0], on[2]], [off[1], off[0], off[2]], sub)
    add("list one key short", sig, on[:2], off[:2], sub)
    # special non-signing keys (signer 0, key 1 is the special one); the signature is made over the lists as they are verified
    sub_sec = _seckey(rng); sub = ref.pubkey_create(sub_sec)
    summed = ref.seckey_tweak_add(w.off_sec[0], sub_sec)
    for nm, off1 in (("offline = -sub", ref.pubkey_negate(sub)), ("offline = sub", sub)):
        offs = [off[0], off1, off[2]]
        add(nm, ref.sign(on, offs, sub, w.on_sec[0], summed, 0), on, offs, sub)
    a = ref.pubkey_combine([off[1], sub])
    on1 = ref.pubkey_negate(ref.pubkey_tweak_mul(a, hashlib.sha256(ref.pubkey_serialize(a)).digest()))
    ons = [on[0], on1, on[2]]
    add("online = -t (offline + sub)", ref.sign(ons, off, sub, w.on_sec[0], summed, 0), ons, off, sub)
    # engine only
    sig, sub = w.sign(ref, rng, 1)
    add("all-zero online key object", sig, [on[0], on[1], b"\0" * 64], off, sub, engine_only=0)
    add("all-zero offline key object", sig, on, [b"\0" * 64, off[1], off[2]], sub, engine_only=0)
    add("all-zero sub key object", sig, on, off, b"\0" * 64, engine_only=0)
    if with_255:                                                     # (its own generator: the cases above do not depend on with_255)
        rng = np.random.default_rng(3304)
        w = Whitelist(ref, rng, 255)
        sig, sub = w.sign(ref, rng, 100)
        add("valid n=255 signer=100", sig, w.online, w.offline, sub)
        add("n=255 last s flipped", _flip(sig, 8 * (len(sig) - 1)), w.online, w.offline, sub)
    return out


def random_items(ref, n_items, seed, lengths=(1, 2, 3, 4, 5, 6, 7, 8), corrupt_every=4):
    """-> list of (sig, online bytes, offline bytes, sub64, expected): seeded signatures of mixed list lengths, every `corrupt_every`-th
    one with a flipped bit somewhere in the signature; verdicts from the reference"""
    rng = np.random.default_rng(seed)
    lists = {n: Whitelist(ref, rng, n) for n in sorted(set(lengths))}
    out = []
    for i in range(n_items):
        w = lists[lengths[int(rng.integers(0, len(lengths)))]]
        sig, sub = w.sign(ref, rng, int(rng.integers(0, w.n)))
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            sig = _flip(sig, int(rng.integers(8, 8 * len(sig))))
        on, off = b"".join(w.online), b"".join(w.offline)
        out.append((sig, on, off, sub, ref.verify(sig, on, off, sub)))
    return out
