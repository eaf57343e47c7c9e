"""ctypes view of the reference's public ECDSA / recovery API in oracle/_ref/libsecp256k1_ref.so (include/secp256k1.h,
include/secp256k1_recovery.h).  Test-only.  ctypes releases the GIL around every call, so the batch helpers use a thread pool."""
import concurrent.futures
import ctypes
import os

import numpy as np

from tests.refapi import REF_PATH, N, P  # noqa: F401

CONTEXT_NONE = 1
EC_COMPRESSED = (1 << 1) | (1 << 8)
EC_UNCOMPRESSED = 1 << 1
THREADS = 16

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class EcdsaRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(REF_PATH)
        L.secp256k1_context_create.restype = _vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        sig = {
            "secp256k1_ecdsa_sign": [_vp, _vp, _vp, _vp, _vp, _vp],
            "secp256k1_ecdsa_verify": [_vp, _vp, _vp, _vp],
            "secp256k1_ecdsa_signature_parse_der": [_vp, _vp, _vp, _sz],
            "secp256k1_ecdsa_signature_parse_compact": [_vp, _vp, _vp],
            "secp256k1_ecdsa_signature_serialize_der": [_vp, _vp, _vp, _vp],
            "secp256k1_ecdsa_signature_serialize_compact": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_create": [_vp, _vp, _vp],
            "secp256k1_ec_pubkey_parse": [_vp, _vp, _vp, _sz],
            "secp256k1_ec_pubkey_serialize": [_vp, _vp, _vp, _vp, ctypes.c_uint],
            "secp256k1_ecdsa_sign_recoverable": [_vp, _vp, _vp, _vp, _vp, _vp],
            "secp256k1_ecdsa_recover": [_vp, _vp, _vp, _vp],
            "secp256k1_ecdsa_recoverable_signature_parse_compact": [_vp, _vp, _vp, _int],
            "secp256k1_ecdsa_recoverable_signature_serialize_compact": [_vp, _vp, _vp, _vp],
        }
        for name, args in sig.items():
            f = getattr(L, name); f.restype = _int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(CONTEXT_NONE)
        assert self.ctx

    # ---- single items (bytes in, bytes out) -----------------------------------------------------------------------------------------
    def pubkey_create(self, seckey32):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ec_pubkey_create(self.ctx, o, seckey32) == 1
        return o.raw

    def pubkey_parse(self, ser):
        """-> 64-byte secp256k1_pubkey object, or None"""
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ec_pubkey_parse(self.ctx, o, bytes(ser), len(ser)) == 1 else None

    def pubkey_serialize(self, obj64, compressed=True):
        o = ctypes.create_string_buffer(65); ln = _sz(65)
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, o, ctypes.byref(ln), obj64, EC_COMPRESSED if compressed else EC_UNCOMPRESSED) == 1
        return o.raw[:ln.value]

    def sign(self, msg32, seckey32):
        """-> 64-byte secp256k1_ecdsa_signature object (low s, RFC 6979 nonce)"""
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ecdsa_sign(self.ctx, o, msg32, seckey32, None, None) == 1
        return o.raw

    def sig_parse_der(self, der):
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ecdsa_signature_parse_der(self.ctx, o, bytes(der), len(der)) == 1 else None

    def sig_parse_compact(self, c64):
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ecdsa_signature_parse_compact(self.ctx, o, bytes(c64)) == 1 else None

    def sig_serialize_der(self, obj64):
        o = ctypes.create_string_buffer(80); ln = _sz(80)
        assert self.lib.secp256k1_ecdsa_signature_serialize_der(self.ctx, o, ctypes.byref(ln), obj64) == 1
        return o.raw[:ln.value]

    def sig_serialize_compact(self, obj64):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ecdsa_signature_serialize_compact(self.ctx, o, obj64) == 1
        return o.raw

    def verify_obj(self, sigobj64, msg32, pkobj64):
        return self.lib.secp256k1_ecdsa_verify(self.ctx, sigobj64, msg32, pkobj64)

    def verify(self, sig, sig_format, msg32, pk, pk_format):
        """what results[i] of secp256k1_ecdsa_verify_batch stands for: both parsers, then secp256k1_ecdsa_verify.  Formats as the engine's."""
        sig = bytes(sig); pk = bytes(pk)
        so = sig if sig_format == 1 else (self.sig_parse_compact(sig) if sig_format == 0 else self.sig_parse_der(sig))
        po = pk if pk_format == 1 else self.pubkey_parse(pk)
        if so is None or po is None:
            return 0
        return self.verify_obj(so, bytes(msg32), po)

    def sign_recoverable(self, msg32, seckey32):
        """-> (compact r|s 64 bytes, recid)"""
        o = ctypes.create_string_buffer(65)
        assert self.lib.secp256k1_ecdsa_sign_recoverable(self.ctx, o, msg32, seckey32, None, None) == 1
        c = ctypes.create_string_buffer(64); rid = _int(0)
        assert self.lib.secp256k1_ecdsa_recoverable_signature_serialize_compact(self.ctx, c, ctypes.byref(rid), o) == 1
        return c.raw, rid.value

    def recoverable_obj(self, compact64, recid):
        """-> 65-byte secp256k1_ecdsa_recoverable_signature object, or None (r or s >= n)"""
        o = ctypes.create_string_buffer(65)
        return o.raw if self.lib.secp256k1_ecdsa_recoverable_signature_parse_compact(self.ctx, o, bytes(compact64), int(recid)) == 1 else None

    def recover(self, compact64, recid, msg32):
        """-> (verdict, 64-byte secp256k1_pubkey object: zero on failure); recid must be 0..3 (the reference aborts otherwise)"""
        ro = self.recoverable_obj(compact64, recid)
        if ro is None:
            return 0, bytes(64)
        o = ctypes.create_string_buffer(64)
        r = self.lib.secp256k1_ecdsa_recover(self.ctx, o, ro, bytes(msg32))
        return r, o.raw

    # ---- batches --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _map(fn, n, threads=THREADS):
        if n < 64:
            return [fn(i) for i in range(n)]
        with concurrent.futures.ThreadPoolExecutor(min(threads, THREADS)) as ex:
            return list(ex.map(fn, range(n), chunksize=max(1, n // (8 * threads))))

    def make(self, n, rng, threads=THREADS):
        """n signatures by n fresh keys -> dict of numpy arrays: msgs (n,32), seckeys (n,32), sigobj (n,64), pkobj (n,64)"""
        sk = rng.integers(0, 256, (n, 32), dtype=np.uint8); sk[:, 0] &= 0x7F; sk[:, 31] |= 1
        msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        skb = [sk[i].tobytes() for i in range(n)]; mb = [msgs[i].tobytes() for i in range(n)]
        out = self._map(lambda i: (self.sign(mb[i], skb[i]), self.pubkey_create(skb[i])), n, threads)
        return {"msgs": msgs, "seckeys": sk, "sigobj": np.frombuffer(b"".join(o[0] for o in out), np.uint8).reshape(n, 64).copy(),
                "pkobj": np.frombuffer(b"".join(o[1] for o in out), np.uint8).reshape(n, 64).copy()}

    def sigs_as(self, sigobj, sig_format):
        """(n,64) signature objects -> what the engine takes for sig_format: an (n,64) array (0, 1) or a list of DER byte strings (2)"""
        n = sigobj.shape[0]
        if sig_format == 1:
            return sigobj.copy()
        if sig_format == 0:
            return np.frombuffer(b"".join(self.sig_serialize_compact(sigobj[i].tobytes()) for i in range(n)), np.uint8).reshape(n, 64).copy()
        return [self.sig_serialize_der(sigobj[i].tobytes()) for i in range(n)]

    def pks_as(self, pkobj, pk_format):
        n = pkobj.shape[0]
        if pk_format == 1:
            return pkobj.copy()
        w = 33 if pk_format == 0 else 65
        return np.frombuffer(b"".join(self.pubkey_serialize(pkobj[i].tobytes(), pk_format == 0) for i in range(n)), np.uint8).reshape(n, w).copy()

    def verify_many(self, sigs, sig_format, msgs, pks, pk_format, threads=THREADS):
        """sigs: (n,64) array or list of DER strings; -> int32[n]"""
        n = len(sigs)
        s = [bytes(sigs[i]) if sig_format == 2 else sigs[i].tobytes() for i in range(n)]
        m = [msgs[i].tobytes() for i in range(n)]; p = [pks[i].tobytes() for i in range(n)]
        return np.array(self._map(lambda i: self.verify(s[i], sig_format, m[i], p[i], pk_format), n, threads), np.int32)

    def make_recoverable(self, n, rng, threads=THREADS):
        """-> msgs (n,32), sigs64 (n,64) compact, recids (n,) uint8, pkobj (n,64): the signers' keys"""
        sk = rng.integers(0, 256, (n, 32), dtype=np.uint8); sk[:, 0] &= 0x7F; sk[:, 31] |= 1
        msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        skb = [sk[i].tobytes() for i in range(n)]; mb = [msgs[i].tobytes() for i in range(n)]
        out = self._map(lambda i: self.sign_recoverable(mb[i], skb[i]) + (self.pubkey_create(skb[i]),), n, threads)
        return (msgs, np.frombuffer(b"".join(o[0] for o in out), np.uint8).reshape(n, 64).copy(), np.array([o[1] for o in out], np.uint8),
                np.frombuffer(b"".join(o[2] for o in out), np.uint8).reshape(n, 64).copy())

    def recover_many(self, sigs64, recids, msgs, threads=THREADS):
        """-> (int32[n], (n,64) pubkey objects).  recid bytes above 3 cannot be put to the reference (its parser aborts): they are 0 by the
        engine's specification and come back as 0 / zero bytes here"""
        n = sigs64.shape[0]
        s = [sigs64[i].tobytes() for i in range(n)]; m = [msgs[i].tobytes() for i in range(n)]; r = [int(x) for x in recids]
        out = self._map(lambda i: self.recover(s[i], r[i], m[i]) if r[i] <= 3 else (0, bytes(64)), n, threads)
        return np.array([o[0] for o in out], np.int32), np.frombuffer(b"".join(o[1] for o in out), np.uint8).reshape(n, 64).copy()


def corrupt(rng, sigs64, msgs, pks, frac):
    """flips one bit of r, s, the message or the key in about n * frac items of (compact or object) 64-byte signatures; returns the item indices"""
    n = sigs64.shape[0]
    idx = np.flatnonzero(rng.integers(0, int(round(1 / frac)), n) == 0)
    for k, i in enumerate(idx):
        what = k % 4
        if what == 0:
            sigs64[i, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        elif what == 1:
            sigs64[i, 32 + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        elif what == 2:
            msgs[i, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        else:
            pks[i, int(rng.integers(0, pks.shape[1]))] ^= 1 << int(rng.integers(0, 8))
    return idx


def _b32(v):
    return int(v).to_bytes(32, "big")


def der_encode(r, s):
    """minimal DER of two non-negative integers (any size: used to build edge cases the reference's serializer cannot produce)"""
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        if b[0] & 0x80:
            b = b"\0" + b
        return b"\x02" + der_len(len(b)) + b
    body = integer(r) + integer(s)
    return b"\x30" + der_len(len(body)) + body


def der_len(n):
    if n < 128:
        return bytes([n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(b)]) + b


def edge_cases(ref, rng):
    """The issue's edge list as (name, sig, sig_format, msg32, pk, pk_format, expected) with expected from the reference, or a literal
    where the reference cannot be asked (marked in the name with '[specified]')."""
    out = []
    b32 = _b32

    def add(name, sig, sf, msg, pk, pf, expected=None):
        out.append((name, bytes(sig), sf, bytes(msg), bytes(pk), pf, ref.verify(sig, sf, msg, pk, pf) if expected is None else expected))

    sk = b32(0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF)
    d = int.from_bytes(sk, "big")
    msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    pko = ref.pubkey_create(sk); pk33 = ref.pubkey_serialize(pko, True); pk65 = ref.pubkey_serialize(pko, False)
    so = ref.sign(msg, sk); c = ref.sig_serialize_compact(so)
    r, s = int.from_bytes(c[:32], "big"), int.from_bytes(c[32:], "big")
    add("valid compact", c, 0, msg, pk33, 0)
    assert out[-1][-1] == 1
    add("r = 0", b32(0) + c[32:], 0, msg, pk33, 0)
    add("s = 0", c[:32] + b32(0), 0, msg, pk33, 0)
    add("r = 0 DER", der_encode(0, s), 2, msg, pk33, 0)
    add("s = 0 DER", der_encode(r, 0), 2, msg, pk33, 0)
    add("r = n compact", b32(N) + c[32:], 0, msg, pk33, 0)
    if r + N < 1 << 256:
        add("r = r + n compact", b32(r + N) + c[32:], 0, msg, pk33, 0)
    add("s = n compact", c[:32] + b32(N), 0, msg, pk33, 0)
    add("s = 2^256 - 1 compact", c[:32] + b32((1 << 256) - 1), 0, msg, pk33, 0)
    add("r >= n DER parses as 0", der_encode(N + 5, s), 2, msg, pk33, 0)
    add("high s compact", c[:32] + b32(N - s), 0, msg, pk33, 0)
    assert out[-1][-1] == 0
    add("high s DER", der_encode(r, N - s), 2, msg, pk33, 0)
    add("high s object", c[:32][::-1] + b32(N - s)[::-1], 1, msg, pko, 1)
    # message hash >= n (reduced silently) and zero
    for name, m in (("msg = n + 7", b32(N + 7)), ("msg = 2^256 - 1", b32((1 << 256) - 1)), ("msg = 0", b32(0)), ("msg = n", b32(N))):
        sm = ref.sig_serialize_compact(ref.sign(m, sk))
        add(name + " valid", sm, 0, m, pk33, 0)
        assert out[-1][-1] == 1
        add(name + " other sig", c, 0, m, pk33, 0)
    add("sig for msg 7 against msg n + 7", ref.sig_serialize_compact(ref.sign(b32(7), sk)), 0, b32(N + 7), pk65, 2)
    assert out[-1][-1] == 1
    # u1 G + u2 P = infinity: P = d G, any r, low s, m = -r d
    for rr, ss in ((r, s), (5, 7), (N - 1, 1)):
        add("R at infinity r=%x.." % (rr >> 240), b32(rr) + b32(ss), 0, b32((-rr * d) % N), pk33, 0)
        assert out[-1][-1] == 0
    # P = G and P = -G
    one = b32(1); g_o = ref.pubkey_create(one); g33 = ref.pubkey_serialize(g_o, True)
    ng_o = ref.pubkey_create(b32(N - 1)); ng33 = ref.pubkey_serialize(ng_o, True)
    for name, key, po, p33 in (("P = G", one, g_o, g33), ("P = -G", b32(N - 1), ng_o, ng33)):
        sg = ref.sig_serialize_compact(ref.sign(msg, key))
        add(name + " valid", sg, 0, msg, p33, 0)
        assert out[-1][-1] == 1
        add(name + " object key", sg, 0, msg, po, 1)
        add(name + " wrong sig", c, 0, msg, p33, 0)
    add("sig by G against -G", ref.sig_serialize_compact(ref.sign(msg, one)), 0, msg, ng33, 0)
    # compressed keys
    for pre in (0x00, 0x04, 0x05, 0x06):
        add("compressed prefix %02x" % pre, c, 0, msg, bytes([pre]) + pk33[1:], 0)
        assert out[-1][-1] == 0
    add("compressed other parity", c, 0, msg, bytes([pk33[0] ^ 1]) + pk33[1:], 0)
    add("compressed x = p", c, 0, msg, b"\x02" + b32(P), 0)
    add("compressed x = p + 1", c, 0, msg, b"\x03" + b32(P + 1), 0)       # (x = 1 is on the curve: only the range check refuses it)
    add("compressed x = 2^256 - 1", c, 0, msg, b"\x02" + b32((1 << 256) - 1), 0)
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    add("compressed x off the curve", c, 0, msg, b"\x02" + b32(x), 0)
    assert out[-1][-1] == 0
    # 65-byte keys
    X, Y = int.from_bytes(pk65[1:33], "big"), int.from_bytes(pk65[33:], "big")
    add("uncompressed valid", c, 0, msg, pk65, 2)
    assert out[-1][-1] == 1
    add("hybrid valid", c, 0, msg, bytes([6 + (Y & 1)]) + pk65[1:], 2)
    assert out[-1][-1] == 1
    add("hybrid wrong parity", c, 0, msg, bytes([7 - (Y & 1)]) + pk65[1:], 2)
    assert out[-1][-1] == 0
    add("uncompressed -y", c, 0, msg, b"\x04" + b32(X) + b32(P - Y), 2)
    add("uncompressed off the curve", c, 0, msg, b"\x04" + b32(X) + b32((Y + 1) % P), 2)
    if Y + P < 1 << 256:
        add("uncompressed y + p", c, 0, msg, b"\x04" + b32(X) + b32(Y + P), 2)
    add("uncompressed y = p", c, 0, msg, b"\x04" + b32(X) + b32(P), 2)
    if X + P < 1 << 256:
        add("uncompressed x + p", c, 0, msg, b"\x04" + b32(X + P) + b32(Y), 2)
    for pre in (0x00, 0x02, 0x03, 0x05, 0x08):
        add("65-byte prefix %02x" % pre, c, 0, msg, bytes([pre]) + pk65[1:], 2)
    add("all-zero key object [specified]", c, 0, msg, bytes(64), 1, expected=0)
    # DER shapes around a valid signature
    der = ref.sig_serialize_der(so)
    add("DER valid", der, 2, msg, pk33, 0)
    assert out[-1][-1] == 1
    body = der[2:]
    variants = {
        "empty": b"", "one byte": b"\x30", "wrong tag": b"\x31" + der[1:], "trailing byte": der + b"\0", "length + 1": der[:1] + bytes([der[1] + 1]) + der[2:],
        "length - 1": der[:1] + bytes([der[1] - 1]) + der[2:], "long-form length": b"\x30\x81" + der[1:2] + body, "indefinite length": b"\x30\x80" + body,
        "length ff": b"\x30\xff" + body, "length 0x88 over": b"\x30\x88" + bytes(8) + body, "length 0x89": b"\x30\x89" + bytes(9) + body,
        "length 0x82 with leading zero": b"\x30\x82\x00" + der[1:2] + body,
        "padded r": b"\x30" + bytes([der[1] + 1]) + b"\x02" + bytes([der[3] + 1]) + b"\0" + der[4:],
        "integer tag 03": der[:2] + b"\x03" + der[3:], "zero-length r": b"\x30" + bytes([len(der) - 4 - der[3] + 2]) + b"\x02\x00" + der[4 + der[3]:],
        "garbage inside tuple": der[:1] + bytes([der[1] + 1]) + der[2:] + b"\0",
        "negative r": der_neg(r, s), "ff-padded r": b"\x30\x08\x02\x02\xff\x80\x02\x02\x00\x01", "r of 33 nonzero bytes": der_encode(1 << 257, s),
        "truncated": der[:-1], "only r": b"\x30" + bytes([2 + der[3]]) + der[2:4 + der[3]],
        "long-form integer length": b"\x30" + bytes([der[1] + 1]) + b"\x02\x81" + der[3:],
    }
    for name, v in variants.items():
        add("DER " + name, v, 2, msg, pk33, 0)
    return out


def der_neg(r, s):
    """DER whose first integer has its top bit set (a negative number): parses, with r = 0"""
    b = int(r | (1 << 255)).to_bytes(32, "big")
    body = b"\x02\x20" + b + der_encode(0, s)[5:]
    return b"\x30" + der_len(len(body)) + body


def recover_cases(ref, rng):
    """(name, sig64, recid, msg32, expected verdict, expected 64 bytes): the recovery edge list; recid bytes above 3 are specified 0"""
    out = []
    b32 = _b32
    msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8))

    def add(name, sig, recid, m=msg):
        v, pk = ref.recover(sig, recid, m) if recid <= 3 else (0, bytes(64))
        out.append((name, bytes(sig), recid, bytes(m), v, pk))

    sk = b32(0xC0FFEE0000000000000000000000000000000000000000000000000000000001)
    c, rid = ref.sign_recoverable(msg, sk)
    for k in range(4):
        add("recid %d (signed with %d)" % (k, rid), c, k)
    add("recid 4", c, 4); add("recid 255", c, 255)
    pmn = P - N
    for rr in (1, 2, 3, pmn - 3, pmn - 2, pmn - 1, pmn, pmn + 1, N - 1):
        for k in range(4):
            add("r = %x recid %d" % (rr, k), b32(rr) + c[32:], k)
    # r whose lift fails
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    add("r off the curve", b32(x) + c[32:], 0); add("r off the curve, odd", b32(x) + c[32:], 1)
    assert out[-1][4] == 0
    add("r = 0", b32(0) + c[32:], 0); add("s = 0", c[:32] + b32(0), 1)
    add("r = n", b32(N) + c[32:], 0); add("s = n", c[:32] + b32(N), 0)
    add("msg = 0", c, rid, b32(0)); add("msg >= n", c, rid, b32(N + 1))
    return out
