"""ctypes view of what the hash tests ask of the reference in oracle/_ref/libsecp256k1_ref.so: secp256k1_tagged_sha256 (include/secp256k1.h),
secp256k1_schnorrsig_sign_custom and secp256k1_schnorrsig_verify (include/secp256k1_schnorrsig.h), with the key calls they need, and the
case lists the CPU and GPU tiers share.  Test-only.  Every expected verdict is the reference's own for exactly the bytes the item gets.

A batch of BIP-340 items with a length each is a dict of numpy arrays:
    sigs (n, 64), blob (the messages back to back), off (n + 1, uint64), pk32 (n, 32) x-only keys, pkobj (n, 64) secp256k1_xonly_pubkey
    objects, expected (n, int32), names (list)"""
import ctypes
import hashlib

import numpy as np

from tests.refapi import REF_PATH

CONTEXT_NONE = 1
TAGS = (b"", b"T", b"BIP0340/challenge", b"t" * 64, b"u" * 65)                     # 0, 1, 17, 64 and 65 bytes
VAR_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 100, 200)
FIXED_LENGTHS = (0, 1, 32, 55, 56, 63, 64, 65, 119, 120)
EXCHANGED = ((0, 1), (31, 32), (33, 63), (64, 65), (100, 200))

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


def sha256(m):
    return hashlib.sha256(bytes(m)).digest()


def sha256d(m):
    return sha256(sha256(m))


def tagged(tag, m):
    t = sha256(tag)
    return sha256(t + t + bytes(m))


def digest(mode, tag, m):
    """mode 0: SHA256, 1: SHA256 of SHA256, 2: tagged"""
    return sha256(m) if mode == 0 else sha256d(m) if mode == 1 else tagged(tag, m)


def pack(items):
    """byte strings -> (blob uint8, offsets uint64[n + 1])"""
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(bytes(x) for x in items), np.uint8).copy(), off


def message(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


class HashRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_tagged_sha256": [_vp, _vp, _vp, _sz, _vp, _sz],
            "secp256k1_keypair_create": [_vp, _vp, _vp],
            "secp256k1_keypair_xonly_pub": [_vp, _vp, _vp, _vp],
            "secp256k1_xonly_pubkey_serialize": [_vp, _vp, _vp],
            "secp256k1_xonly_pubkey_parse": [_vp, _vp, _vp],
            "secp256k1_schnorrsig_sign_custom": [_vp, _vp, _vp, _sz, _vp, _vp],
            "secp256k1_schnorrsig_verify": [_vp, _vp, _vp, _sz, _vp],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx

    def tagged_sha256(self, tag, msg):
        o = ctypes.create_string_buffer(32)
        assert self.lib.secp256k1_tagged_sha256(self.ctx, o, bytes(tag), len(tag), bytes(msg), len(msg)) == 1
        return o.raw

    def keypair(self, seckey32):
        """-> (96-byte keypair, 32-byte x-only key, 64-byte secp256k1_xonly_pubkey object)"""
        kp = ctypes.create_string_buffer(96)
        assert self.lib.secp256k1_keypair_create(self.ctx, kp, bytes(seckey32)) == 1
        obj = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_keypair_xonly_pub(self.ctx, obj, None, kp) == 1
        x = ctypes.create_string_buffer(32)
        assert self.lib.secp256k1_xonly_pubkey_serialize(self.ctx, x, obj) == 1
        return kp.raw, x.raw, obj.raw

    def sign(self, msg, keypair96):
        """secp256k1_schnorrsig_sign_custom with the default nonce function and no auxiliary randomness"""
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_schnorrsig_sign_custom(self.ctx, o, bytes(msg), len(msg), bytes(keypair96), None) == 1
        return o.raw

    def verify(self, sig64, msg, pkobj64):
        return self.lib.secp256k1_schnorrsig_verify(self.ctx, bytes(sig64), bytes(msg), len(msg), bytes(pkobj64))

    def verify_x32(self, sig64, msg, pk32):
        """what pk_format 0 stands for: secp256k1_xonly_pubkey_parse, then the verification"""
        obj = ctypes.create_string_buffer(64)
        if self.lib.secp256k1_xonly_pubkey_parse(self.ctx, obj, bytes(pk32)) != 1:
            return 0
        return self.verify(sig64, msg, obj.raw)

    # ---- batches -----------------------------------------------------------------------------------------------------------------------
    def signed(self, rng, length):
        """one fresh key and one message of `length` bytes -> (sig64, msg, pk32, pkobj64)"""
        sk = bytearray(message(rng, 32)); sk[0] &= 0x7F; sk[31] |= 1
        kp, x, obj = self.keypair(bytes(sk))
        m = message(rng, length)
        return self.sign(m, kp), m, x, obj

    def finish(self, rows):
        """rows of (name, sig64, the bytes the item gets, pk32, pkobj64) -> the batch, every verdict asked of the reference"""
        blob, off = pack([r[2] for r in rows])
        n = len(rows)
        return {"names": [r[0] for r in rows], "sigs": np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(n, 64).copy(), "blob": blob, "off": off,
                "pk32": np.frombuffer(b"".join(r[3] for r in rows), np.uint8).reshape(n, 32).copy(),
                "pkobj": np.frombuffer(b"".join(r[4] for r in rows), np.uint8).reshape(n, 64).copy(),
                "expected": np.array([self.verify(r[1], r[2], r[4]) for r in rows], np.int32)}

    def var_cases(self, seed=3401):
        """The edge list of secp256k1_schnorrsig_verify_batch_var.  Per length of VAR_LENGTHS four signatures as they are and four corrupted
        ones (one message byte flipped, the message shortened by one byte -- both only where there is a byte --, s flipped, r flipped); per
        pair of EXCHANGED two neighbours whose messages lie back to back with their two lengths exchanged.  40 items as signed, 48 not."""
        rng = np.random.default_rng(seed)
        rows = []
        for ln in VAR_LENGTHS:
            for k in range(4):
                s, m, x, o = self.signed(rng, ln)
                rows.append((f"len {ln} valid {k}", s, m, x, o))
            if ln:
                s, m, x, o = self.signed(rng, ln)
                at = int(rng.integers(0, ln)); bad = bytearray(m); bad[at] ^= 1 << int(rng.integers(0, 8))
                rows.append((f"len {ln} message byte {at} flipped", s, bytes(bad), x, o))
                s, m, x, o = self.signed(rng, ln)
                rows.append((f"len {ln} message shortened by one byte", s, m[:-1], x, o))
            for name, at in (("s", 32 + int(rng.integers(0, 32))), ("r", int(rng.integers(0, 32)))):
                s, m, x, o = self.signed(rng, ln)
                bad = bytearray(s); bad[at] ^= 1 << int(rng.integers(0, 8))
                rows.append((f"len {ln} {name} flipped", bytes(bad), m, x, o))
        for la, lb in EXCHANGED:
            sa, ma, xa, oa = self.signed(rng, la)
            sb, mb, xb, ob = self.signed(rng, lb)
            both = ma + mb
            rows.append((f"lengths {la} and {lb} exchanged, first", sa, both[:lb], xa, oa))
            rows.append((f"lengths {la} and {lb} exchanged, second", sb, both[lb:], xb, ob))
        return self.finish(rows)

    def var_random(self, n, seed, max_len=300):
        """n seeded items of 0 .. max_len bytes, every fourth corrupted (message bit, length, s, r in turn)"""
        rng = np.random.default_rng(seed)
        rows = []
        for i in range(n):
            ln = int(rng.integers(0, max_len + 1))
            s, m, x, o = self.signed(rng, ln)
            if i % 4 == 3:
                what = (i // 4) % 4
                if what == 0 and ln:
                    bad = bytearray(m); bad[int(rng.integers(0, ln))] ^= 1 << int(rng.integers(0, 8)); m = bytes(bad)
                elif what == 1:
                    m = m[:-1] if ln else b"\x00"
                else:
                    bad = bytearray(s); bad[(32 if what == 2 else 0) + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8)); s = bytes(bad)
            rows.append((f"random {i}", s, m, x, o))
        return self.finish(rows)
