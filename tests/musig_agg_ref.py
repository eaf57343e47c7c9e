"""A Python statement of the four MuSig2 calls of csrc/musig_agg.h as include/secp256k1_zkp_amd.h documents them: key aggregation
(secp256k1_musig_pubkey_agg, src/modules/musig/keyagg_impl.h:156-215 of the reference), the two cache tweaks (:231-273), nonce
aggregation (session_impl.h:493-531) and signature aggregation (:779-805), with the edge lists and seeded pools their tests share.
Test-only.  pubkey_agg, tweak_add and nonce_agg over points are those of tests/musig_ref.py; what is added here is partial_sig_agg, a
pubkey_agg that groups identical keys (a large set drawn from 8 distinct points costs 8 multiplications), the verdict-and-bytes
functions, and the rows.

What ties the model to the reference is tests/golden/musig_agg_vectors.json, written by tests/golden/make_musig_agg_golden.py: every
answer in it was returned by the reference's own functions; the module's BIP-327 rows are recorded in full, and the rows built here
from seeds by the reference's verdict and one SHA-256 over their inputs and the reference's verdict and output bytes (to_json /
from_json below), which keeps the file small and still pins every byte.

Rows.  A field that does not exist in a representation is None, as in tests/musig_ref.py:
    key aggregation   (name, keys33, keys64, keys65, verdict, cache197, agg_pk64)       the key list in the three pk_formats
    cache tweak       (name, cache197, tweak32, xonly_byte, verdict, cache_out197, pubkey_out64)
    nonce aggregation (name, pubnonces66, pubnonces132, verdict, aggnonce66, aggnonce132)
    signature agg.    (name, session133, sigs32, sigs36, verdict, sig64)
An aggregate key at infinity cannot be constructed (every coefficient is a hash over all keys), so that refusal has no row."""
import functools
import hashlib

import numpy as np

from tests import musig_ref as M
from tests.musig_ref import (BAD, INF, N, P, MAGIC_PUBNONCE, MAGIC_SESSION, MAGIC_SIG, b32, g_mul, lift_x, obj_pt, parse33, parse_full, pt_add, pt_mul, pt_neg, pt_obj,
                             ser33, _flip, _int, _rand_scalar, _set)

PK_BYTES = {0: 33, 1: 64, 2: 65}
KEYAGG_LIST_TAG = "KeyAgg list"
KEYAGG_INPUTS, TWEAK_INPUTS, NONCE_INPUTS, SIG_INPUTS = 3, 3, 2, 3          # fields behind the name that are inputs
NO_KEYAGG = (0, bytes(197), bytes(64))


def ser65(a, prefix=4):
    return bytes([prefix]) + b32(a[0]) + b32(a[1])


def split(blob, size):
    blob = bytes(blob)
    assert len(blob) % size == 0
    return [blob[i:i + size] for i in range(0, len(blob), size)]


def parse_key(k, pk_format):
    """a point, or BAD; format 1: the object as it is, all-zero x refused"""
    if pk_format == 0:
        return parse33(k)
    if pk_format == 2:
        return parse_full(k)
    return BAD if bytes(k[:32]) == bytes(32) else obj_pt(k)


# ---- the four calls over parsed inputs -----------------------------------------------------------------------------------------------------
def pubkey_agg_grouped(pks, second):
    """the cache of a key list whose second key is given (INF: none); identical keys share one multiplication.  None: infinity"""
    pks_hash = M.tagged(KEYAGG_LIST_TAG, b"".join(ser33(p) for p in pks))
    count = {}
    for p in pks:
        count[p] = count.get(p, 0) + 1
    Q = INF
    for p, c in count.items():
        Q = pt_add(Q, pt_mul(c * M.keyagg_coef(pks_hash, p, second) % N, p))
    return None if Q is INF else M.cache_pack(Q, second, pks_hash, 0, 0)


def partial_sig_agg(session, shares):
    """secp256k1_musig_partial_sig_agg over integers: the 64-byte signature"""
    s = _int(session[101:133]) % N
    for t in shares:
        s = (s + t) % N
    return bytes(session[5:37]) + b32(s)


# ---- verdict and bytes, as the header documents them ---------------------------------------------------------------------------------------
def keyagg_bytes(keys, pk_format):
    """(verdict, cache197, agg_pk64) of one key set given as the concatenation of its keys"""
    ks = split(keys, PK_BYTES[pk_format])
    pts = [parse_key(k, pk_format) for k in ks]
    if not ks or BAD in pts:
        return NO_KEYAGG
    same = (lambda a, b: a[1:] == b[1:]) if pk_format == 2 else (lambda a, b: a == b)
    second = next((pts[i] for i in range(1, len(ks)) if not same(ks[i], ks[0])), INF)
    cache = pubkey_agg_grouped(pts, second)
    if cache is None:
        return NO_KEYAGG
    Q = obj_pt(cache[4:68])
    return 1, cache, pt_obj(Q if Q[1] % 2 == 0 else pt_neg(Q))


def tweak_bytes(cache, tweak32, xonly_byte):
    """(verdict, cache_out197, pubkey_out64)"""
    c = M.tweak_add(cache, tweak32, xonly_byte) if xonly_byte in (0, 1) else None
    return (0, bytes(197), bytes(64)) if c is None else (1, c, c[4:68])


def nonce_agg_bytes(pubnonces, nonce_format):
    """(verdict, aggnonce66, aggnonce132)"""
    ns = split(pubnonces, 132 if nonce_format else 66)
    if nonce_format:
        Rs = [BAD if n[:4] != MAGIC_PUBNONCE else (obj_pt(n[4:68]), obj_pt(n[68:132])) for n in ns]
    else:
        Rs = [(parse33(n[:33]), parse33(n[33:])) for n in ns]
        Rs = [BAD if BAD in r else r for r in Rs]
    if not ns or BAD in Rs:
        return 0, bytes(66), bytes(132)
    R1, R2 = M.nonce_agg(Rs)
    return 1, M.aggnonce_ser(R1, R2), M.aggnonce_obj(R1, R2)


def sig_agg_bytes(session, sigs, sig_format):
    """(verdict, sig64)"""
    ss = split(sigs, 36 if sig_format else 32)
    if sig_format:
        vals = [BAD if s[:4] != MAGIC_SIG else _int(s[4:]) % N for s in ss]
    else:
        vals = [BAD if _int(s) >= N else _int(s) for s in ss]
    if not ss or BAD in vals or bytes(session[:4]) != MAGIC_SESSION:
        return 0, bytes(64)
    return 1, partial_sig_agg(session, vals)


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------
def make_krow(name, pts=None, keys33=None, keys64=None, keys65=None):
    """pts (a list of points) gives all three representations; the raw fields override or replace them"""
    if pts is not None:
        keys33 = b"".join(ser33(p) for p in pts) if keys33 is None else keys33
        keys64 = b"".join(pt_obj(p) for p in pts) if keys64 is None else keys64
        keys65 = b"".join(ser65(p) for p in pts) if keys65 is None else keys65
    got = {keyagg_bytes(k, f) for f, k in enumerate((keys33, keys64, keys65)) if k is not None}
    assert len(got) == 1, (name, got)
    return (name, keys33, keys64, keys65) + got.pop()


def make_trow(name, cache, tweak32, xonly_byte):
    return (name, bytes(cache), bytes(tweak32), xonly_byte) + tweak_bytes(cache, tweak32, xonly_byte)


def make_nrow(name, Rs=None, ser=None, obj=None):
    if Rs is not None:
        ser = b"".join(M.pubnonce_ser(*r) for r in Rs) if ser is None else ser
        obj = b"".join(M.pubnonce_obj(*r) for r in Rs) if obj is None else obj
    got = {nonce_agg_bytes(b, f) for f, b in enumerate((ser, obj)) if b is not None}
    assert len(got) == 1, (name, got)
    return (name, ser, obj) + got.pop()


def make_srow(name, session, shares=None, ser=None, obj=None):
    if shares is not None:
        ser = b"".join(b32(s) for s in shares) if ser is None else ser
        obj = b"".join(M.sig_obj(s) for s in shares) if obj is None else obj
    got = {sig_agg_bytes(session, b, f) for f, b in enumerate((ser, obj)) if b is not None}
    assert len(got) == 1, (name, got)
    return (name, bytes(session), ser, obj) + got.pop()


def off_curve_x(near):
    return next(x for x in range(near, near + 200) if lift_x(x, 0) is None)


@functools.lru_cache(maxsize=None)
def _edge_points():
    rng = np.random.default_rng(6621)
    sks = [_rand_scalar(rng) for _ in range(10)]
    return sks, [g_mul(d) for d in sks]


@functools.lru_cache(maxsize=None)
def keyagg_edges():
    """the smallest shapes where each stage of key aggregation can go wrong; verdicts in KEYAGG_EDGE_REFUSED"""
    _, pts = _edge_points()
    Pp, Q, R = pts[0], pts[1], pts[2]
    bad = b"\x02" + b32(off_curve_x(Pp[0]))
    E = [make_krow("one key", [Pp]),
         make_krow("two keys (the second's coefficient is 1)", [Pp, Q]),
         make_krow("all keys equal (second infinite, all doublings)", [Pp, Pp, Pp, Pp]),
         make_krow("[P, P, Q]: the second key is index 2", [Pp, Pp, Q]),
         make_krow("[P, Q, Q]", [Pp, Q, Q]),
         make_krow("[P, -P, Q]", [Pp, pt_neg(Pp), Q]),
         make_krow("[P, Q, P, Q, R]", [Pp, Q, Pp, Q, R]),
         make_krow("key 1 a hybrid encoding of key 0's point, Q after it", keys65=ser65(Pp) + ser65(Pp, 6 + (Pp[1] & 1)) + ser65(Q)),
         make_krow("hybrid encodings throughout", keys65=b"".join(ser65(a, 6 + (a[1] & 1)) for a in (Pp, Q, R))),
         make_krow("hybrid prefix of the wrong parity", keys65=ser65(Pp) + ser65(Q, 7 - (Q[1] & 1))),
         make_krow("uncompressed key off the curve", keys65=ser65(Pp) + ser65((Q[0], Q[1] ^ 2))),
         make_krow("an all-zero key object", keys64=pt_obj(Pp) + bytes(64) + pt_obj(Q)),
         make_krow("compressed x >= p", keys33=ser33(Pp) + b"\x02" + b32(P + 1)),
         make_krow("x off the curve", keys33=ser33(Pp) + bad),
         make_krow("prefix 04 in format 0", keys33=ser33(Pp) + b"\x04" + ser33(Q)[1:]),
         make_krow("a refused key in first position", keys33=bad + ser33(Q) + ser33(R)),
         make_krow("a refused key in middle position", keys33=ser33(Pp) + bad + ser33(R)),
         make_krow("a refused key in last position", keys33=ser33(Pp) + ser33(Q) + bad),
         make_krow("an empty set", keys33=b"", keys64=b"", keys65=b"")]
    for m in (63, 64, 65, 130):                                                  # around the default fan-in; drawn from 8 points
        E.append(make_krow("%d keys from 8 points" % m, [pts[(5 * i + i // 8) % 8] for i in range(m)]))
    for m in range(2, 10):                                                       # up to four passes at fan-in 2
        E.append(make_krow("%d distinct keys" % m, pts[:m]))
    return E


KEYAGG_EDGE_REFUSED = ("hybrid prefix of the wrong parity", "uncompressed key off the curve", "an all-zero key object", "compressed x >= p", "x off the curve",
                       "prefix 04 in format 0", "a refused key in first position", "a refused key in middle position", "a refused key in last position", "an empty set")


def aggregate_secret(sks, cache):
    """d with d*G = the untweaked cache's key"""
    c = M.cache_unpack(cache)
    return sum(M.keyagg_coef(c["pks_hash"], g_mul(d), c["second"]) * d for d in sks) % N


@functools.lru_cache(maxsize=None)
def tweak_edges():
    rng = np.random.default_rng(6622)
    sks, _ = _edge_points()
    shapes = M.cache_shapes(rng, sks[:2])
    E = []
    for (shape, par), sc in sorted(shapes.items()):
        t = b32(_rand_scalar(rng))
        for xo in (0, 1):
            E.append(make_trow("cache %s, aggregate key %s, %s tweak" % (shape, par, "x-only" if xo else "plain"), sc.cache, t, xo))
    sc = shapes[("plain tweak", "odd")]
    for nm, t in (("tweak 0", 0), ("tweak n - 1", N - 1), ("tweak n", N), ("tweak 2^256 - 1", 2 ** 256 - 1)):
        for xo in (0, 1):
            E.append(make_trow("%s, xonly %d" % (nm, xo), sc.cache, t.to_bytes(32, "big"), xo))
    for par in ("odd", "even"):
        u = shapes[("untweaked", par)]
        d = aggregate_secret(u.sks, u.cache)
        assert g_mul(d) == M.cache_unpack(u.cache)["pk"]
        E.append(make_trow("tweak = minus the aggregate secret (%s key), plain: infinity" % par, u.cache, b32(N - d), 0))
        E.append(make_trow("the same after the x-only negation (%s key): infinity" % par, u.cache, b32(d if par == "odd" else N - d), 1))
        E.append(make_trow("plus the aggregate secret (%s key), plain: the doubling" % par, u.cache, b32(d), 0))
    t = b32(_rand_scalar(rng))
    E.append(make_trow("wrong magic", _set(sc.cache, 2, b"\xbc"), t, 0))
    E.append(make_trow("xonly byte 2", sc.cache, t, 2))
    E.append(make_trow("xonly byte 255", sc.cache, t, 255))
    for v in (2, 3):
        E.append(make_trow("parity_acc byte %d, x-only tweak" % v, _set(shapes[("x-only tweak", "odd")].cache, 164, bytes([v])), t, 1))
    return E


def _tweak_refused(name):
    return any(s in name for s in ("tweak n,", "tweak 2^256", "infinity", "wrong magic", "xonly byte"))


@functools.lru_cache(maxsize=None)
def nonce_edges():
    rng = np.random.default_rng(6623)
    Rs = [(g_mul(_rand_scalar(rng)), g_mul(_rand_scalar(rng))) for _ in range(65)]
    neg = lambda r: (pt_neg(r[0]), pt_neg(r[1]))
    xoff = off_curve_x(Rs[0][0][0])
    s2 = b"".join(M.pubnonce_ser(*r) for r in Rs[:2])
    E = [make_nrow("%d pubnonces" % m, Rs[:m]) for m in (1, 2, 3, 64, 65)]
    E += [make_nrow("two equal pubnonces (the doubling)", [Rs[0], Rs[0]]),
          make_nrow("R and -R in the first column only", [Rs[0], (pt_neg(Rs[0][0]), Rs[1][1])]),
          make_nrow("R and -R in the second column only", [Rs[0], (Rs[1][0], pt_neg(Rs[0][1]))]),
          make_nrow("R and -R in both columns", [Rs[0], neg(Rs[0])]),
          make_nrow("R, S, -R, -S in both columns", [Rs[0], Rs[1], neg(Rs[0]), neg(Rs[1])]),
          make_nrow("R, -R, S", [Rs[0], neg(Rs[0]), Rs[1]]),
          make_nrow("wrong magic", obj=M.pubnonce_obj(*Rs[0]) + _set(M.pubnonce_obj(*Rs[1]), 3, b"\xa1")),
          make_nrow("an invalid second point", ser=s2[:99] + b"\x02" + b32(xoff)),
          make_nrow("an invalid first point of the first pubnonce", ser=b"\x05" + s2[1:]),
          make_nrow("33 zero bytes", ser=s2[:66] + bytes(33) + s2[99:]),
          make_nrow("an empty range", ser=b"", obj=b"")]
    return E


NONCE_EDGE_REFUSED = ("wrong magic", "an invalid second point", "an invalid first point of the first pubnonce", "33 zero bytes", "an empty range")


@functools.lru_cache(maxsize=None)
def sig_edges():
    rng = np.random.default_rng(6624)
    sks, _ = _edge_points()
    plain = M.Scenario(rng, sks[:3])
    tw = M.Scenario(rng, sks[:3], tweaks=[(_rand_scalar(rng), 1)])
    assert _int(tw.session[101:]) != 0 and _int(plain.session[101:]) == 0
    E = []
    for nm, sc in (("untweaked session", plain), ("a non-zero s_part (tweaked cache)", tw)):
        E.append(make_srow(nm, sc.session, [sc.share(i) for i in range(3)]))
        E.append(make_srow(nm + ", one share", sc.session, [sc.share(0)]))
    E += [make_srow("a sum that wraps mod n", tw.session, [N - 1, N - 2, N - 3]),
          make_srow("shares 0", plain.session, [0, 0]),
          make_srow("object s = n (reduced)", plain.session, obj=M.sig_obj(5) + MAGIC_SIG + b32(N)),
          make_srow("serialised s = n (refused)", plain.session, ser=b32(5) + b32(N)),
          make_srow("wrong magic: session", _set(plain.session, 0, b"\x9c"), [1, 2]),
          make_srow("wrong magic: partial signature", plain.session, obj=M.sig_obj(1) + b"\xeb\xfb\x1a\x33" + b32(2)),
          make_srow("an empty range", plain.session, ser=b"", obj=b"")]
    return E


SIG_EDGE_REFUSED = ("serialised s = n (refused)", "wrong magic: session", "wrong magic: partial signature", "an empty range")


# ---- seeded random rows (the fixture's 64 per call) ----------------------------------------------------------------------------------------
FIXTURE_SEED = 6625


@functools.lru_cache(maxsize=None)
def random_rows(k, seed, corrupt_every=4):
    """(key aggregation, tweak, nonce, signature) rows, k each; every corrupt_every-th row carries one flipped bit in its serialised
    inputs (objects are made from what still parses: a point inside an object is never off the curve here)"""
    rng = np.random.default_rng(seed)
    K, T, Nn, S = [], [], [], []
    for i in range(k):
        bad = bool(corrupt_every) and i % corrupt_every == corrupt_every - 1
        # key aggregation: 1..6 keys, now and then a repeated one
        m = 1 + int(rng.integers(0, 6))
        sks = [_rand_scalar(rng) for _ in range(m)]
        if m > 2 and i % 3 == 0:
            sks[int(rng.integers(1, m))] = sks[0]
        pts = [g_mul(d) for d in sks]
        ser = b"".join(ser33(p) for p in pts)
        if bad:
            ser = _flip(ser, int(rng.integers(0, 8 * len(ser))))
            pts = [parse33(x) for x in split(ser, 33)]
        K.append(make_krow("random %d" % i, None if BAD in pts else pts, keys33=ser))
        # tweak: on the untweaked cache, then on the tweaked one
        cache = M.pubkey_agg([g_mul(d) for d in sks])
        t1, x1, t2, x2 = b32(_rand_scalar(rng)), int(rng.integers(0, 2)), b32(_rand_scalar(rng)), int(rng.integers(0, 2))
        if i % 2:
            cache = M.tweak_add(cache, t1, x1)
        blob = cache[:4] + cache[164:] + t2                                      # what a flipped bit may touch: magic, parity_acc, tweak, the new tweak
        if bad:
            blob = _flip(blob, int(rng.integers(0, 8 * 69)))
        T.append(make_trow("random %d" % i, blob[:4] + cache[4:164] + blob[4:37], blob[37:], x2))
        # nonce aggregation: 1..5 pubnonces
        Rs = [(g_mul(_rand_scalar(rng)), g_mul(_rand_scalar(rng))) for _ in range(1 + int(rng.integers(0, 5)))]
        ser = b"".join(M.pubnonce_ser(*r) for r in Rs)
        if bad:
            ser = _flip(ser, int(rng.integers(0, 8 * len(ser))))
            Rs = [(parse33(x[:33]), parse33(x[33:])) for x in split(ser, 66)]
        Nn.append(make_nrow("random %d" % i, None if any(BAD in r for r in Rs) else Rs, ser=ser))
        # signature aggregation: a session of 2..4 signers
        sc = M.Scenario(rng, [_rand_scalar(rng) for _ in range(2 + int(rng.integers(0, 3)))], tweaks=[(_rand_scalar(rng), i % 2)] if i % 3 else ())
        blob = sc.session + b"".join(b32(sc.share(j)) for j in range(len(sc.sks)))
        if bad:
            blob = _flip(blob, int(rng.integers(0, 8 * len(blob))))
        vals = [_int(x) for x in split(blob[133:], 32)]
        S.append(make_srow("random %d" % i, blob[:133], None if any(v >= N for v in vals) else vals, ser=blob[133:]))
    return K, T, Nn, S


# ---- the fixture file ----------------------------------------------------------------------------------------------------------------------
def _generated(which):
    edges = (keyagg_edges, tweak_edges, nonce_edges, sig_edges)[which]()
    return {r[0]: r for r in list(edges) + list(random_rows(64, FIXTURE_SEED)[which])}


def _digest(fields):
    h = hashlib.sha256()
    for x in fields:
        x = bytes([x]) if isinstance(x, int) else x
        h.update(b"\xff" if x is None else len(x).to_bytes(4, "big") + bytes(x))
    return h.hexdigest()


def _hx(x):
    return bytes(x).hex() if isinstance(x, (bytes, bytearray)) else x


def _un(x):
    return bytes.fromhex(x) if isinstance(x, str) else x


def to_json(rows, which, n_in):
    """rows whose answers are the reference's.  A row this file can build again is recorded as [name, the reference's verdict, SHA-256
    over the row's inputs and the reference's verdict and output bytes]; any other row (the module's own vectors) in full, as hex."""
    gen = _generated(which)
    return [[r[0], r[1 + n_in], _digest(r[1:])] if r[0] in gen else [r[0]] + [_hx(x) for x in r[1:]] for r in rows]


def from_json(rows, which, n_in):
    """the full rows again.  A rebuilt row -- its inputs and the model's answer to them -- is checked against the recorded digest: the
    bytes handed out are the model's, and they answer the inputs the reference was asked as the reference did, or this fails"""
    gen, out = _generated(which), []
    for r in rows:
        if r[0] in gen:
            g = gen[r[0]]
            assert g[1 + n_in] == r[1] and _digest(g[1:]) == r[2], "%r built now is not the row the reference answered, or the model's answer is not the reference's" % r[0]
            out.append(tuple(g))
        else:
            out.append((r[0],) + tuple(_un(x) for x in r[1:]))
    return out


# ---- pools for the batch tests -------------------------------------------------------------------------------------------------------------
POOL_SEED = 6620


@functools.lru_cache(maxsize=None)
def keyagg_pool(seed=POOL_SEED, n_sets=64):
    """n_sets sets of compressed keys: (keys33, corrupted, (verdict, cache, agg_pk), the uncorrupted set's (verdict, cache, agg_pk)).
    Each set has 1 + rng.integers(0, 9) fresh keys; every eighth set (i % 8 == 5) gets its last key set to its first; every fourth
    (i % 4 == 3) one flipped bit in its concatenated compressed keys.  Draw order: per set the size, then the keys, then the bit."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sets):
        m = 1 + int(rng.integers(0, 9))
        pts = [g_mul(_rand_scalar(rng)) for _ in range(m)]
        if i % 8 == 5:
            pts[-1] = pts[0]
        ser = b"".join(ser33(p) for p in pts)
        clean = keyagg_bytes(ser, 0)
        bad = i % 4 == 3
        if bad:
            ser = _flip(ser, int(rng.integers(0, 8 * len(ser))))
        out.append((ser, bad, keyagg_bytes(ser, 0) if bad else clean, clean))
    return out


def batch(sets, pk_format=0):
    """(concatenated keys, offsets in keys) of a list of key blobs"""
    off = np.zeros(len(sets) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) // PK_BYTES[pk_format] for s in sets])
    return b"".join(sets), off
