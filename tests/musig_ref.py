"""A Python statement of secp256k1_musig_partial_sig_verify and secp256k1_musig_nonce_process over plain integers
(src/modules/musig/session_impl.h:544-638, :716-777, keyagg_impl.h:19-130 of the reference), of what builds their inputs
(pubkey_agg, the two cache tweaks, nonce_agg, partial_sign), the object layouts, and the edge lists the MuSig tests share.  Test-only.

The reference library the other oracles use (oracle/_ref) is built without the musig module, so this model is the oracle of the CPU
tier; what ties it to the reference is tests/golden/musig_vectors.json, whose verdicts and sessions the reference's own functions
returned when tests/golden/make_musig_golden.py wrote the file (the rows built here from seeds are recorded there by the SHA-256 of
their inputs, next to the reference's answers: to_json / from_json below).

A verify row is the tuple
    (name, sig_ser, sig_obj, nonce_ser, nonce_obj, pk_ser, pk_obj, cache, session, verdict)
and a process row
    (name, nonce_ser, nonce_obj, msg32, cache, adaptor, verdict, session_out)
A field that does not exist in a representation is None: rows that exist only as objects are the wrong magics, the object holding
s = n and the all-zero key; rows that exist only serialised are the invalid encodings.  verify_formats() / process_formats() hand a
row out in a format combination, or None.

R1 + b*R2 = infinity in nonce processing (the final nonce falling back to G) cannot be constructed with R2 finite: b is a hash over
R1 and R2, so it would take a discrete logarithm or a hash preimage.  The fallback is reached by the both-infinite item only."""
import functools
import hashlib

import numpy as np

from tests.adaptor_ref import pt_add, pt_neg, pt_mul, lift_x, ser33, b32, G, INF, P, N, _rand_scalar, _flip, _jac_add_affine      # noqa: F401

BAD = "bad"                                   # a point that does not parse (INF is None)
MAGIC_CACHE = bytes([0xf4, 0xad, 0xbb, 0xdf])
MAGIC_PUBNONCE = bytes([0xf5, 0x7a, 0x3d, 0xa0])
MAGIC_AGGNONCE = bytes([0xa8, 0xb7, 0xe4, 0x67])
MAGIC_SESSION = bytes([0x9d, 0xed, 0xe9, 0x17])
MAGIC_SIG = bytes([0xeb, 0xfb, 0x1a, 0x32])
TAGS = ("KeyAgg coefficient", "MuSig/noncecoef", "BIP0340/challenge")


_G_POWERS = []


def g_mul(k):
    """k*G from the 256 points 2^i G: additions only, about three times as fast as pt_mul (the tests build thousands of keys and nonces)"""
    if not _G_POWERS:
        a = G
        for _ in range(256):
            _G_POWERS.append(a); a = pt_add(a, a)
    r, k = (0, 1, 0), k % N
    for i in range(k.bit_length()):
        if (k >> i) & 1:
            r = _jac_add_affine(r, _G_POWERS[i])
    if r[2] == 0:
        return INF
    zi = pow(r[2], -1, P)
    return (r[0] * zi * zi % P, r[1] * zi * zi * zi % P)


def tagged(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


def _int(b):
    return int.from_bytes(bytes(b), "big")


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def parse33(b):
    """secp256k1_eckey_pubkey_parse of 33 bytes: a point, or BAD"""
    b = bytes(b)
    if len(b) != 33 or b[0] not in (2, 3):
        return BAD
    a = lift_x(_int(b[1:]), b[0] & 1)
    return BAD if a is None else a


def parse_ext(b):
    return INF if bytes(b) == bytes(33) else parse33(b)


def ser_ext(a):
    return bytes(33) if a is INF else ser33(a)


def pt_obj(a):
    """secp256k1_ge_to_bytes: x, y as 32 little-endian bytes each"""
    return a[0].to_bytes(32, "little") + a[1].to_bytes(32, "little")


def pt_obj_ext(a):
    return bytes(64) if a is INF else pt_obj(a)


def obj_pt(b):
    return (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little"))


def obj_pt_ext(b):
    return INF if bytes(b) == bytes(64) else obj_pt(b)


def parse_full(b):
    """65 bytes, uncompressed or hybrid"""
    b = bytes(b)
    if len(b) != 65 or b[0] not in (4, 6, 7):
        return BAD
    x, y = _int(b[1:33]), _int(b[33:])
    if x >= P or y >= P or (y * y - x * x * x - 7) % P:
        return BAD
    if b[0] != 4 and (y & 1) != (b[0] & 1):
        return BAD
    return (x, y)


def cache_pack(pk, second, pks_hash, parity_acc, tweak):
    return MAGIC_CACHE + pt_obj(pk) + pt_obj_ext(second) + bytes(pks_hash) + bytes([parity_acc]) + b32(tweak)


def cache_unpack(c):
    """secp256k1_keyagg_cache_load: None on a wrong magic"""
    c = bytes(c)
    assert len(c) == 197
    if c[:4] != MAGIC_CACHE:
        return None
    return dict(pk=obj_pt(c[4:68]), second=obj_pt_ext(c[68:132]), pks_hash=c[132:164], parity_acc=c[164] & 1, tweak=_int(c[165:197]) % N)


def pubnonce_ser(R1, R2):
    return ser33(R1) + ser33(R2)


def pubnonce_obj(R1, R2):
    return MAGIC_PUBNONCE + pt_obj(R1) + pt_obj(R2)


def aggnonce_ser(R1, R2):
    return ser_ext(R1) + ser_ext(R2)


def aggnonce_obj(R1, R2):
    return MAGIC_AGGNONCE + pt_obj_ext(R1) + pt_obj_ext(R2)


def sig_obj(s):
    return MAGIC_SIG + b32(s)


# ---- what builds the inputs ---------------------------------------------------------------------------------------------------------------
def keyagg_coef(pks_hash, pk, second):
    if second is not INF and pk == second:
        return 1
    return _int(tagged("KeyAgg coefficient", bytes(pks_hash) + ser33(pk))) % N


def pubkey_agg(pks):
    """secp256k1_musig_pubkey_agg: the cache of a list of points"""
    second = next((p for p in pks[1:] if p != pks[0]), INF)
    pks_hash = tagged("KeyAgg list", b"".join(ser33(p) for p in pks))
    Q = INF
    for p in pks:
        Q = pt_add(Q, pt_mul(keyagg_coef(pks_hash, p, second), p))
    assert Q is not INF
    return cache_pack(Q, second, pks_hash, 0, 0)


def tweak_add(cache, tweak32, xonly):
    """secp256k1_musig_pubkey_ec_tweak_add / _xonly_tweak_add: the new cache, or None"""
    c = cache_unpack(cache)
    t = _int(tweak32)
    if c is None or t >= N:
        return None
    pk, acc, tw = c["pk"], c["parity_acc"], c["tweak"]
    if xonly and pk[1] & 1:
        pk, acc, tw = pt_neg(pk), acc ^ 1, (N - tw) % N
    tw = (tw + t) % N
    pk = pt_add(pk, g_mul(t))
    if pk is INF:
        return None
    return cache_pack(pk, c["second"], c["pks_hash"], acc, tw)


def nonce_agg(pubnonces):
    R1 = R2 = INF
    for a, b in pubnonces:
        R1, R2 = pt_add(R1, a), pt_add(R2, b)
    return R1, R2


@functools.lru_cache(maxsize=4096)
def nonce_process(R1, R2, msg32, cache, adaptor=None):
    """the session of an aggregate nonce given as points (INF allowed), or None.  adaptor: a 64-byte object or None"""
    c = cache_unpack(cache)
    if c is None:
        return None
    if adaptor is not None:
        if bytes(adaptor[:32]) == bytes(32):                  # secp256k1_pubkey_load: ARG_CHECK(!fe_is_zero(x))
            return None
        R1 = pt_add(R1, obj_pt(adaptor))
    pkx = b32(c["pk"][0])
    b = _int(tagged("MuSig/noncecoef", ser_ext(R1) + ser_ext(R2) + pkx + bytes(msg32))) % N
    F = pt_add(R1, pt_mul(b, R2))
    if F is INF:
        F = G
    e = _int(tagged("BIP0340/challenge", b32(F[0]) + pkx + bytes(msg32))) % N
    sp = 0
    if c["tweak"]:
        sp = e * c["tweak"] % N
        if c["pk"][1] & 1:
            sp = (N - sp) % N
    return MAGIC_SESSION + bytes([F[1] & 1]) + b32(F[0]) + b32(b) + b32(e) + b32(sp)


def process_bytes(nonce, nonce_format, msg32, cache, adaptor=None):
    """(verdict, 133 bytes) as secp256k1_musig_nonce_process_batch documents them"""
    nonce = bytes(nonce)
    if nonce_format == 1:
        R = None if nonce[:4] != MAGIC_AGGNONCE else (obj_pt_ext(nonce[4:68]), obj_pt_ext(nonce[68:132]))
    else:
        R = (parse_ext(nonce[:33]), parse_ext(nonce[33:]))
        R = None if BAD in R else R
    s = None if R is None else nonce_process(R[0], R[1], msg32, cache, adaptor)
    return (0, bytes(133)) if s is None else (1, s)


def verify_terms(cache, session, Ppt):
    """(e', sigma, b) of the verification equation  s*G == e'*P + sigma*(R1 + b*R2)"""
    c = cache_unpack(cache)
    b, e = _int(session[37:69]) % N, _int(session[69:101]) % N
    e1 = e * keyagg_coef(c["pks_hash"], Ppt, c["second"]) % N
    if (c["pk"][1] & 1) != c["parity_acc"]:
        e1 = (N - e1) % N
    return e1, (-1 if session[4] else 1), b


def partial_sign(d, k1, k2, cache, session):
    """secp256k1_musig_partial_sign with the nonces as arguments"""
    e1, sigma, b = verify_terms(cache, session, g_mul(d))
    return (e1 * d + sigma * (k1 + b * k2)) % N


def verify_bytes(sig, sig_format, nonce, nonce_format, pk, pk_format, cache, session):
    """what secp256k1_musig_partial_sig_verify_batch documents for one item; returns 0 or 1"""
    sig, nonce, pk, cache, session = bytes(sig), bytes(nonce), bytes(pk), bytes(cache), bytes(session)
    if sig_format == 1:
        if sig[:4] != MAGIC_SIG:
            return 0
        s = _int(sig[4:]) % N
    else:
        s = _int(sig)
        if s >= N:
            return 0
    if nonce_format == 1:
        if nonce[:4] != MAGIC_PUBNONCE:
            return 0
        R1, R2 = obj_pt(nonce[4:68]), obj_pt(nonce[68:132])
    else:
        R1, R2 = parse33(nonce[:33]), parse33(nonce[33:])
        if BAD in (R1, R2):
            return 0
    if pk_format == 1:
        if pk[:32] == bytes(32):
            return 0
        Ppt = obj_pt(pk)
    else:
        Ppt = parse33(pk) if pk_format == 0 else parse_full(pk)
        if Ppt == BAD:
            return 0
    if cache[:4] != MAGIC_CACHE or session[:4] != MAGIC_SESSION:
        return 0
    return _verify_points(s, R1, R2, Ppt, cache, session)


@functools.lru_cache(maxsize=4096)
def _verify_points(s, R1, R2, Ppt, cache, session):
    """the verification equation on parsed inputs (cached: a row is asked once per format combination it exists in)"""
    e1, sigma, b = verify_terms(cache, session, Ppt)
    Rj = pt_add(R1, pt_mul(b, R2))
    if sigma < 0:
        Rj = pt_neg(Rj)
    return int(pt_add(pt_add(g_mul(N - s), pt_mul(e1, Ppt)), Rj) is INF)


# ---- rows -------------------------------------------------------------------------------------------------------------------------------
def verify_formats(row, sf, nf, pf):
    """(sig, nonce, pk) of a verify row in the format combination, or None where the row does not exist in it"""
    sig = row[2] if sf else row[1]
    nonce = row[4] if nf else row[3]
    if pf == 1:
        pk = row[6]
    elif pf == 0:
        pk = row[5]
    else:
        a = BAD if row[5] is None else parse33(row[5])
        pk = None if a == BAD else b"\x04" + b32(a[0]) + b32(a[1])
    return None if sig is None or nonce is None or pk is None else (sig, nonce, pk)


def process_formats(row, nf):
    return row[2] if nf else row[1]


ALL_VERIFY_FORMATS = [(sf, nf, pf) for sf in (0, 1) for nf in (0, 1) for pf in (0, 1, 2)]


def make_vrow(name, cache, session, sig_ser=None, sig_o=None, nonce_ser=None, nonce_o=None, pk_ser=None, pk_o=None, s=None, R=None, Ppt=None):
    """s (an integer below n), R = (R1, R2) and Ppt give both representations; the raw fields override or replace them.  The verdict is
    the model's, and every combination the row exists in must give the same one"""
    if s is not None:
        sig_ser, sig_o = b32(s), sig_obj(s)
    if R is not None:
        nonce_ser, nonce_o = pubnonce_ser(*R), pubnonce_obj(*R)
    if Ppt is not None:
        pk_ser, pk_o = ser33(Ppt), pt_obj(Ppt)
    row = [name, sig_ser, sig_o, nonce_ser, nonce_o, pk_ser, pk_o, bytes(cache), bytes(session)]
    got = set()
    for f in ALL_VERIFY_FORMATS:
        a = verify_formats(row, *f)
        if a is not None:
            got.add(verify_bytes(a[0], f[0], a[1], f[1], a[2], f[2], cache, session))
    assert len(got) == 1, (name, got)
    return tuple(row) + (got.pop(),)


def make_prow(name, msg, cache, nonce_ser=None, nonce_o=None, R=None, adaptor=None):
    if R is not None:
        nonce_ser, nonce_o = aggnonce_ser(*R), aggnonce_obj(*R)
    got = set()
    for nf, nonce in ((0, nonce_ser), (1, nonce_o)):
        if nonce is not None:
            got.add(process_bytes(nonce, nf, msg, cache, adaptor))
    assert len(got) == 1, (name, got)
    v, sess = got.pop()
    return (name, nonce_ser, nonce_o, bytes(msg), bytes(cache), None if adaptor is None else bytes(adaptor), v, sess)


def _rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())


class Scenario:
    """one signing session: keys (secret scalars), optional tweaks [(t, xonly)], the signers' nonces, the message"""

    def __init__(self, rng, sks, tweaks=(), msg=None):
        self.sks = list(sks)
        self.pks = [g_mul(d) for d in self.sks]
        self.cache = pubkey_agg(self.pks)
        for t, xonly in tweaks:
            self.cache = tweak_add(self.cache, b32(t), xonly)
            assert self.cache is not None
        self.ks = [(_rand_scalar(rng), _rand_scalar(rng)) for _ in self.sks]
        self.Rs = [(g_mul(a), g_mul(b)) for a, b in self.ks]
        self.agg = nonce_agg(self.Rs)
        self.msg = _rand_bytes(rng, 32) if msg is None else msg
        self.session = nonce_process(self.agg[0], self.agg[1], self.msg, self.cache)

    def share(self, i, cache=None, session=None):
        return partial_sign(self.sks[i], self.ks[i][0], self.ks[i][1], cache or self.cache, session or self.session)

    def row(self, name, i, **kw):
        return make_vrow(name, self.cache, self.session, s=self.share(i), R=self.Rs[i], Ppt=self.pks[i], **kw)

    def q_odd(self):
        return cache_unpack(self.cache)["pk"][1] & 1


def cache_shapes(rng, base_sks):
    """{(shape, 'odd' | 'even'): Scenario}: the four cache shapes, each with an aggregate key of odd and of even y"""
    out = {}
    for shape, xo in (("untweaked", ()), ("plain tweak", (0,)), ("x-only tweak", (1,)), ("both tweaks", (0, 1))):
        for j in range(1, 200):
            sc = Scenario(rng, base_sks + ([j] if not xo else []), tweaks=[(1000 * j + k, x) for k, x in enumerate(xo)])
            key = (shape, "odd" if sc.q_odd() else "even")
            out.setdefault(key, sc)
            if (shape, "odd") in out and (shape, "even") in out:
                break
    assert len(out) == 8
    return out


def _set(b, at, val):
    b = bytearray(b); b[at:at + len(val)] = val; return bytes(b)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(verify rows, process rows); the verdicts EDGE_VERDICTS names are asserted by tests/test_cpu_musig.py on the model and were
    returned by the reference when the fixture was written"""
    rng = np.random.default_rng(6601)
    x0, x1, x2 = (_rand_scalar(rng) for _ in range(3))
    V, Pr = [], []
    sc = Scenario(rng, [x0, x1, x2])
    # ---- who the signer is
    V.append(sc.row("signer is the second key (mu = 1)", 1))
    V.append(sc.row("signer is the first key", 0))
    V.append(sc.row("signer is the third key", 2))
    V.append(Scenario(rng, [x0, x0]).row("all keys equal (second_pk infinite)", 1))
    V.append(Scenario(rng, [x0, x1, N - x1]).row("P = -second_pk (hashes, is not 1)", 2))
    # ---- the four cache shapes, aggregate keys of odd and of even y
    shapes = cache_shapes(rng, [x0, x1])
    for (shape, par), s in sorted(shapes.items()):
        V.append(s.row("cache %s, aggregate key %s" % (shape, par), 0))
        Pr.append(make_prow("cache %s, aggregate key %s" % (shape, par), s.msg, s.cache, R=s.agg))
    # ---- the loads
    for v in (0, 1, 2):
        sess = _set(sc.session, 4, bytes([v]))
        V.append(make_vrow("nonce parity byte %d" % v, sc.cache, sess, s=sc.share(0, session=sess), R=sc.Rs[0], Ppt=sc.pks[0]))
    tw = shapes[("x-only tweak", "odd")]
    for v in (2, 3):
        cache = _set(tw.cache, 164, bytes([v]))
        V.append(make_vrow("parity_acc byte %d" % v, cache, tw.session, s=tw.share(0, cache=cache), R=tw.Rs[0], Ppt=tw.pks[0]))
    s0 = sc.share(0)
    V.append(make_vrow("s + 1", sc.cache, sc.session, s=(s0 + 1) % N, R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("s = 0", sc.cache, sc.session, s=0, R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("serialised s = n", sc.cache, sc.session, sig_ser=b32(N), R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("object s = n", sc.cache, sc.session, sig_o=MAGIC_SIG + b32(N), R=sc.Rs[0], Ppt=sc.pks[0]))
    # a share that is valid with s = 0: the verifier takes the session as given, so R1 = -(e' d + sigma b k2) sigma * G makes it so
    e1, sigma, b = verify_terms(sc.cache, sc.session, sc.pks[0])
    k2 = _rand_scalar(rng)
    k1 = (-sigma * e1 * x0 - b * k2) % N
    Rz = (g_mul(k1), g_mul(k2))
    assert partial_sign(x0, k1, k2, sc.cache, sc.session) == 0
    V.append(make_vrow("s = 0, valid", sc.cache, sc.session, s=0, R=Rz, Ppt=sc.pks[0]))
    V.append(make_vrow("object s = n, valid as 0", sc.cache, sc.session, sig_o=MAGIC_SIG + b32(N), R=Rz, Ppt=sc.pks[0]))
    V.append(make_vrow("serialised s = n where 0 is valid", sc.cache, sc.session, sig_ser=b32(N), R=Rz, Ppt=sc.pks[0]))
    V.append(make_vrow("wrong magic: partial signature", sc.cache, sc.session, sig_o=b"\xeb\xfb\x1a\x33" + b32(s0), R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("wrong magic: pubnonce", sc.cache, sc.session, s=s0, nonce_o=_set(pubnonce_obj(*sc.Rs[0]), 0, b"\xf5\x7a\x3d\xa1"), Ppt=sc.pks[0]))
    V.append(make_vrow("wrong magic: cache", _set(sc.cache, 0, b"\xf5"), sc.session, s=s0, R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("wrong magic: session", sc.cache, _set(sc.session, 3, b"\x18"), s=s0, R=sc.Rs[0], Ppt=sc.pks[0]))
    V.append(make_vrow("all-zero key object", sc.cache, sc.session, s=s0, R=sc.Rs[0], pk_o=bytes(64)))
    px = ser33(sc.pks[0])
    V.append(make_vrow("compressed key: x >= p", sc.cache, sc.session, s=s0, R=sc.Rs[0], pk_ser=b"\x02" + b32(P + 1)))
    xoff = next(x for x in range(sc.pks[0][0], sc.pks[0][0] + 100) if lift_x(x, 0) is None)
    V.append(make_vrow("compressed key: x off the curve", sc.cache, sc.session, s=s0, R=sc.Rs[0], pk_ser=b"\x02" + b32(xoff)))
    V.append(make_vrow("compressed key: prefix 04", sc.cache, sc.session, s=s0, R=sc.Rs[0], pk_ser=b"\x04" + px[1:]))
    ns = pubnonce_ser(*sc.Rs[0])
    V.append(make_vrow("serialised pubnonce: R1 invalid", sc.cache, sc.session, s=s0, nonce_ser=b"\x02" + b32(xoff) + ns[33:], Ppt=sc.pks[0]))
    V.append(make_vrow("serialised pubnonce: R2 invalid", sc.cache, sc.session, s=s0, nonce_ser=ns[:33] + b"\x05" + ns[34:], Ppt=sc.pks[0]))
    V.append(make_vrow("serialised pubnonce: 33 zero bytes", sc.cache, sc.session, s=s0, nonce_ser=bytes(33) + ns[33:], Ppt=sc.pks[0]))
    # ---- the fallback path of the joint form: a zero scalar, P = +-R2
    for nm, at in (("b = 0", 37), ("e = 0", 69)):
        sess = _set(sc.session, at, bytes(32))
        V.append(make_vrow("hand-made session with " + nm, sc.cache, sess, s=sc.share(0, session=sess), R=sc.Rs[0], Ppt=sc.pks[0]))
    for nm, kk in (("R2 = P", x0), ("R2 = -P", N - x0)):
        R = (sc.Rs[0][0], g_mul(kk))
        V.append(make_vrow(nm, sc.cache, sc.session, s=partial_sign(x0, sc.ks[0][0], kk, sc.cache, sc.session), R=R, Ppt=sc.pks[0]))
    # ---- infinity and doubling around T = -s*G + sigma*R1 and J = e'*P + sigma*b*R2
    sj = _rand_scalar(rng)
    sessj = _set(sc.session, 37, b32((-sigma * e1) % N))                      # sigma*b = -e' and R2 = P: J is infinity
    Rj = (g_mul(sigma * sj % N), sc.pks[0])
    V.append(make_vrow("b' = -e', R2 = P, s*G = sigma*R1: J and T infinite, valid", sc.cache, sessj, s=sj, R=Rj, Ppt=sc.pks[0]))
    V.append(make_vrow("T infinite alone", sc.cache, sc.session, s=sj, R=(g_mul(sigma * sj % N), sc.Rs[0][1]), Ppt=sc.pks[0]))
    V.append(make_vrow("J infinite alone", sc.cache, sessj, s=sj, R=(sc.Rs[0][0], sc.pks[0]), Ppt=sc.pks[0]))
    V.append(make_vrow("J == T (the doubling in the last comparison)", sc.cache, sc.session, s=(N - s0) % N, R=(pt_neg(sc.Rs[0][0]), sc.Rs[0][1]), Ppt=sc.pks[0]))
    V.append(make_vrow("R1 = s*G", sc.cache, sc.session, s=s0, R=(g_mul(s0), sc.Rs[0][1]), Ppt=sc.pks[0]))
    sd = (e1 * x0 + sigma * b * sc.ks[0][1]) * pow(2, -1, N) % N               # R1 = -sigma*s*G: T = -2s*G, and J = 2s*G
    V.append(make_vrow("R1 = -sigma*s*G: the doubling inside T, valid", sc.cache, sc.session, s=sd, R=(g_mul(-sigma * sd % N), sc.Rs[0][1]), Ppt=sc.pks[0]))

    # ---- nonce processing
    A = g_mul(_rand_scalar(rng))
    Pr.append(make_prow("both aggregate points infinite (the final nonce is G)", sc.msg, sc.cache, R=(INF, INF)))
    Pr.append(make_prow("only R1 infinite", sc.msg, sc.cache, R=(INF, sc.agg[1])))
    Pr.append(make_prow("only R2 infinite", sc.msg, sc.cache, R=(sc.agg[0], INF)))
    Pr.append(make_prow("adaptor", sc.msg, sc.cache, R=sc.agg, adaptor=pt_obj(A)))
    Pr.append(make_prow("adaptor = -R1", sc.msg, sc.cache, R=sc.agg, adaptor=pt_obj(pt_neg(sc.agg[0]))))
    Pr.append(make_prow("adaptor = R1 (the doubling)", sc.msg, sc.cache, R=sc.agg, adaptor=pt_obj(sc.agg[0])))
    Pr.append(make_prow("adaptor on an infinite R1", sc.msg, sc.cache, R=(INF, sc.agg[1]), adaptor=pt_obj(A)))
    Pr.append(make_prow("adaptor = -R1, R2 infinite (the final nonce is G)", sc.msg, sc.cache, R=(sc.agg[0], INF), adaptor=pt_obj(pt_neg(sc.agg[0]))))
    Pr.append(make_prow("all-zero adaptor object", sc.msg, sc.cache, R=sc.agg, adaptor=bytes(64)))
    Pr.append(make_prow("wrong magic: cache", sc.msg, _set(sc.cache, 1, b"\xae"), R=sc.agg))
    Pr.append(make_prow("wrong magic: aggregate nonce", sc.msg, sc.cache, nonce_o=_set(aggnonce_obj(*sc.agg), 0, b"\xf5\x7a\x3d\xa0")))
    na = aggnonce_ser(*sc.agg)
    Pr.append(make_prow("serialised aggregate nonce: R1 invalid", sc.msg, sc.cache, nonce_ser=b"\x02" + b32(xoff) + na[33:]))
    Pr.append(make_prow("serialised aggregate nonce: R2 invalid", sc.msg, sc.cache, nonce_ser=na[:33] + b"\x03" + b32(P)))
    return V, Pr


# every other edge item: 0
EDGE_VERDICTS = {nm: 1 for nm in (
    ["signer is the second key (mu = 1)", "signer is the first key", "signer is the third key", "all keys equal (second_pk infinite)", "P = -second_pk (hashes, is not 1)"] +
    ["cache %s, aggregate key %s" % (s, p) for s in ("untweaked", "plain tweak", "x-only tweak", "both tweaks") for p in ("odd", "even")] +
    ["nonce parity byte 0", "nonce parity byte 1", "nonce parity byte 2", "parity_acc byte 2", "parity_acc byte 3", "s = 0, valid", "object s = n, valid as 0",
     "hand-made session with b = 0", "hand-made session with e = 0", "R2 = P", "R2 = -P", "b' = -e', R2 = P, s*G = sigma*R1: J and T infinite, valid",
     "R1 = -sigma*s*G: the doubling inside T, valid"])}
EDGE_PROCESS_FAILS = ("all-zero adaptor object", "wrong magic: cache", "wrong magic: aggregate nonce", "serialised aggregate nonce: R1 invalid",
                      "serialised aggregate nonce: R2 invalid")                  # every other process edge item: 1
# edge items the joint form must decline (a zero scalar, or P = +-R2 meeting its own x), and dead items (scalars zeroed)
FALLBACK_ROWS = ("hand-made session with b = 0", "hand-made session with e = 0", "wrong magic: cache", "wrong magic: session")


@functools.lru_cache(maxsize=None)
def random_items(k, seed, corrupt_every=4):
    """(verify rows, process rows), k each: seeded sessions of 2..4 signers, with and without tweaks; every corrupt_every-th row carries
    one flipped bit somewhere in its serialised inputs and objects (a bit the call does not read leaves the verdict alone: the model says)"""
    rng = np.random.default_rng(seed)
    V, Pr = [], []
    for i in range(k):
        ns = 2 + int(rng.integers(0, 3))
        tweaks = [(_rand_scalar(rng), int(rng.integers(0, 2))) for _ in range(int(rng.integers(0, 3)))]
        sc = Scenario(rng, [_rand_scalar(rng) for _ in range(ns)], tweaks=tweaks)
        j = int(rng.integers(0, ns))
        sig, nonce, pk, cache, sess = b32(sc.share(j)), pubnonce_ser(*sc.Rs[j]), ser33(sc.pks[j]), sc.cache, sc.session
        adaptor = pt_obj(g_mul(_rand_scalar(rng))) if i % 2 else None
        an, msg, pc = aggnonce_ser(*sc.agg), sc.msg, sc.cache
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            blob = _flip(sig + nonce + pk + cache + sess, int(rng.integers(0, 8 * 461)))
            sig, nonce, pk, cache, sess = blob[:32], blob[32:98], blob[98:131], blob[131:328], blob[328:461]
            blob = _flip(an + msg + pc, int(rng.integers(0, 8 * 295)))
            an, msg, pc = blob[:66], blob[66:98], blob[98:295]
        s = _int(sig)
        R = (parse33(nonce[:33]), parse33(nonce[33:]))
        Pp = parse33(pk)
        V.append(make_vrow("random %d" % i, cache, sess, sig_ser=sig, sig_o=sig_obj(s) if s < N else None, nonce_ser=nonce, nonce_o=None if BAD in R else pubnonce_obj(*R),
                           pk_ser=pk, pk_o=None if Pp == BAD else pt_obj(Pp)))
        Ra = (parse_ext(an[:33]), parse_ext(an[33:]))
        Pr.append(make_prow("random %d" % i, msg, pc, nonce_ser=an, nonce_o=None if BAD in Ra else aggnonce_obj(*Ra), adaptor=adaptor))
    return V, Pr


# ---- the fixture file ------------------------------------------------------------------------------------------------------------------------
FIXTURE_SEED = 6602
VERIFY_INPUTS, PROCESS_INPUTS = 8, 5          # fields behind the name that are inputs; the rest are the reference's answers


def _hx(x):
    return bytes(x).hex() if isinstance(x, (bytes, bytearray)) else x


def _un(x):
    return bytes.fromhex(x) if isinstance(x, str) else x


def _digest(row, n_in):
    h = hashlib.sha256()
    for x in row[1:1 + n_in]:
        h.update(b"\xff" if x is None else len(x).to_bytes(2, "big") + bytes(x))
    return h.hexdigest()


def _generated(n_in):
    """the rows this file builds from seeds, by name: the edge list and the fixture's 64 random rows"""
    k = 0 if n_in == VERIFY_INPUTS else 1
    return {r[0]: r for r in edge_cases()[k] + random_items(64, FIXTURE_SEED)[k]}


def to_json(rows, n_in):
    """A row this file can build again is recorded as [name, SHA-256 of its inputs, the reference's answers]; any other row (the
    module's own vectors) in full, as hex."""
    gen = _generated(n_in)
    return [[r[0], _digest(r, n_in)] + [_hx(x) for x in r[1 + n_in:]] if r[0] in gen else [r[0]] + [_hx(x) for x in r[1:]] for r in rows]


def from_json(rows, n_in):
    """the full rows again: inputs rebuilt here and checked against the recorded digest, answers as recorded"""
    gen, out = _generated(n_in), []
    for r in rows:
        if r[0] in gen:
            g = gen[r[0]]
            assert _digest(g, n_in) == r[1], "the inputs of %r built now are not the ones the reference was asked" % r[0]
            out.append(tuple(g[:1 + n_in]) + tuple(_un(x) for x in r[2:]))
        else:
            out.append((r[0],) + tuple(_un(x) for x in r[1:]))
    return out


# ---- pools for the batch tests: many shares on a few sessions ---------------------------------------------------------------------------
def shared_pool(k, seed, n_sessions=8, signers=5, corrupt_every=8):
    """(caches, sessions, items): n_sessions signing sessions of `signers` keys each and k shares on them, all serialised:
    items[i] = (sig32, pubnonce66, key33, session index, verdict).  Every corrupt_every-th share carries one flipped bit in its own
    131 bytes (the pairs are shared and stay as they are), so it may also stop parsing; the verdicts are the model's."""
    rng = np.random.default_rng(seed)
    scs = [Scenario(rng, [_rand_scalar(rng) for _ in range(signers)], tweaks=[(_rand_scalar(rng), t % 2)] if t % 3 else ()) for t in range(n_sessions)]
    items = []
    for i in range(k):
        S = i % n_sessions; sc = scs[S]; j = (i // n_sessions) % signers
        # a fresh second nonce per share: the verifier takes the pubnonce as given, so the share only has to match it
        k2 = _rand_scalar(rng); R = (sc.Rs[j][0], g_mul(k2))
        blob = b32(partial_sign(sc.sks[j], sc.ks[j][0], k2, sc.cache, sc.session)) + pubnonce_ser(*R) + ser33(sc.pks[j])
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            blob = _flip(blob, int(rng.integers(0, 8 * 131)))
        sig, nonce, pk = blob[:32], blob[32:98], blob[98:131]
        items.append((sig, nonce, pk, S, verify_bytes(sig, 0, nonce, 0, pk, 0, sc.cache, sc.session)))
    return [s.cache for s in scs], [s.session for s in scs], items


def process_pool(k, seed, n_sessions=8, corrupt_every=8):
    """k items (aggnonce66, msg32, cache197, adaptor64, (verdict, session) without the adaptor, (verdict, session) with it); every
    corrupt_every-th one carries one flipped bit in its aggregate nonce or message"""
    rng = np.random.default_rng(seed)
    scs = [Scenario(rng, [_rand_scalar(rng) for _ in range(3)], tweaks=[(_rand_scalar(rng), t % 2)] if t % 3 else ()) for t in range(n_sessions)]
    ads = [pt_obj(g_mul(_rand_scalar(rng))) for _ in range(n_sessions)]
    out = []
    for i in range(k):
        sc = scs[i % n_sessions]
        blob = aggnonce_ser(*sc.agg) + hashlib.sha256(b"process pool %d %d" % (seed, i)).digest()
        if corrupt_every and i % corrupt_every == corrupt_every - 1:
            blob = _flip(blob, int(rng.integers(0, 8 * 98)))
        an, msg, ad = blob[:66], blob[66:], ads[(i // n_sessions) % n_sessions]
        out.append((an, msg, sc.cache, ad, process_bytes(an, 0, msg, sc.cache), process_bytes(an, 0, msg, sc.cache, ad)))
    return out


def chain_items(k, seed, n_sessions=8, corrupt_every=8):
    """k items for nonce processing followed by verification with one pair per share: (aggnonce66, msg32, cache197, sig32, pubnonce66,
    key33, verdict).  The share is made under the session the model computes for the item; every corrupt_every-th share has one bit flipped."""
    rng = np.random.default_rng(seed)
    scs = [Scenario(rng, [_rand_scalar(rng) for _ in range(3)], tweaks=[(_rand_scalar(rng), t % 2)] if t % 3 else ()) for t in range(n_sessions)]
    out = []
    for i in range(k):
        sc = scs[i % n_sessions]; j = (i // n_sessions) % 3
        msg = hashlib.sha256(b"chain %d %d" % (seed, i)).digest()
        sess = nonce_process(sc.agg[0], sc.agg[1], msg, sc.cache)
        s = sc.share(j, session=sess)
        bad = bool(corrupt_every) and i % corrupt_every == corrupt_every - 1
        if bad:
            s ^= 1 << int(rng.integers(0, 255))
            s %= N
        out.append((aggnonce_ser(*sc.agg), msg, sc.cache, b32(s), pubnonce_ser(*sc.Rs[j]), ser33(sc.pks[j]), 0 if bad else 1))
    return out
