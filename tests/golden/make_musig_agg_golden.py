#!/usr/bin/env python3
"""Writes tests/golden/musig_agg_vectors.json: recorded inputs of secp256k1_musig_pubkey_agg, the two cache tweaks,
secp256k1_musig_nonce_agg and secp256k1_musig_partial_sig_agg with the caches, x-only keys, aggregate nonces and signatures the
reference's own functions returned when the file was written.

Run once in the build container:   python tests/golden/make_musig_agg_golden.py [--time]
As tests/golden/make_musig_golden.py (whose MusigRef this script extends): the unmodified reference, with the musig, extrakeys and
schnorrsig modules switched on, is compiled into a temporary directory outside the repository, loaded with ctypes with an
illegal-argument callback that does nothing, asked, and removed.  Nothing compiled from the reference is kept, and no test compiles
anything.

Contents: the module's own BIP-327 data (musig_key_agg_vector with its valid and error cases, musig_nonce_agg_vector,
musig_tweak_vector and musig_sig_agg_vector, read from src/modules/musig/vectors.h as data when this script runs), the edge lists of
tests/musig_agg_ref.py and 64 seeded random rows per call, and the "KeyAgg list" midstate constant of keyagg_impl.h:65-68 as data.
Serialised inputs go through the reference's parsers (an input that does not parse gives verdict 0); objects are handed over as they
are.  Where the reference returns 0 the recorded outputs are zero bytes, which is what the engine documents (the reference leaves the
cache of a refused tweak as it was); an xonly byte other than 0 or 1 has no counterpart in the reference and is recorded as the
engine documents it.  The model of tests/musig_agg_ref.py must agree with the reference on every row, in every byte, or nothing is
written.  The module's rows are recorded in full; a row the model file builds again from its seeds is recorded as its name, the
reference's verdict and one SHA-256 over its inputs and the reference's verdict and output bytes.  --time also prints the reference's time per call on one core of this machine."""
import ctypes
import json
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_musig_golden import MusigRef, REF, c_initializer      # noqa: E402


class MusigAggRef(MusigRef):
    def __init__(self):
        super().__init__()
        vp, cp, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
        L = self.lib
        L.secp256k1_musig_partial_sig_agg.argtypes = [vp, vp, cp, vp, sz]
        L.secp256k1_musig_aggnonce_serialize.argtypes = [vp, vp, cp]
        L.secp256k1_musig_pubkey_ec_tweak_add.argtypes = [vp, vp, vp, cp]
        L.secp256k1_musig_pubkey_xonly_tweak_add.argtypes = [vp, vp, vp, cp]

    @staticmethod
    def _ptrs(objs, size):
        bufs = [ctypes.create_string_buffer(bytes(o), size) for o in objs]
        return bufs, (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])

    def key65(self, key65):
        return self._parse(self.lib.secp256k1_ec_pubkey_parse, 64, key65, 65)

    def keyagg(self, key_objs):
        """(verdict, cache, agg_pk); zero bytes where the reference returns 0"""
        bufs, arr = self._ptrs(key_objs, 64)
        cache, agg = ctypes.create_string_buffer(197), ctypes.create_string_buffer(64)
        v = self.lib.secp256k1_musig_pubkey_agg(self.ctx, agg, cache, arr, len(bufs))
        return (1, cache.raw, agg.raw) if v == 1 else (0, bytes(197), bytes(64))

    def tweak_full(self, cache, tweak32, xonly):
        c, pk = ctypes.create_string_buffer(bytes(cache), 197), ctypes.create_string_buffer(64)
        fn = self.lib.secp256k1_musig_pubkey_xonly_tweak_add if xonly else self.lib.secp256k1_musig_pubkey_ec_tweak_add
        v = fn(self.ctx, pk, c, bytes(tweak32))
        return (1, c.raw, pk.raw) if v == 1 else (0, bytes(197), bytes(64))

    def nonce_agg_full(self, pubnonce_objs):
        bufs, arr = self._ptrs(pubnonce_objs, 132)
        out = ctypes.create_string_buffer(132)
        if self.lib.secp256k1_musig_nonce_agg(self.ctx, out, arr, len(bufs)) != 1:
            return 0, bytes(66), bytes(132)
        ser = ctypes.create_string_buffer(66)
        assert self.lib.secp256k1_musig_aggnonce_serialize(self.ctx, ser, out.raw) == 1
        return 1, ser.raw, out.raw

    def sig_agg(self, session, sig_objs):
        bufs, arr = self._ptrs(sig_objs, 36)
        out = ctypes.create_string_buffer(64)
        v = self.lib.secp256k1_musig_partial_sig_agg(self.ctx, out, bytes(session), arr, len(bufs))
        return (1, out.raw) if v == 1 else (0, bytes(64))


def _one(answers, name):
    assert len(set(answers)) == 1, "the reference's answers differ between the representations of " + name
    return answers[0]


def ask_keyagg(ref, row):
    from tests import musig_agg_ref as A
    got = []
    for f, parse in ((0, ref.key), (1, lambda k: k), (2, ref.key65)):
        if row[1 + f] is None:
            continue
        objs = [parse(k) for k in A.split(row[1 + f], A.PK_BYTES[f])]
        got.append((0, bytes(197), bytes(64)) if any(o is None for o in objs) else ref.keyagg(objs))
    return _one(got, row[0])


def ask_tweak(ref, row):
    if row[3] not in (0, 1):
        return 0, bytes(197), bytes(64)                      # (no such call in the reference: the engine's contract)
    return ref.tweak_full(row[1], row[2], row[3])


def ask_nonce(ref, row):
    from tests import musig_agg_ref as A
    got = []
    for f, parse in ((0, ref.pubnonce), (1, lambda k: k)):
        if row[1 + f] is None:
            continue
        objs = [parse(k) for k in A.split(row[1 + f], 132 if f else 66)]
        got.append((0, bytes(66), bytes(132)) if any(o is None for o in objs) else ref.nonce_agg_full(objs))
    return _one(got, row[0])


def ask_sig(ref, row):
    from tests import musig_agg_ref as A
    got = []
    for f, parse in ((0, ref.sig), (1, lambda k: k)):
        if row[2 + f] is None:
            continue
        objs = [parse(k) for k in A.split(row[2 + f], 36 if f else 32)]
        got.append((0, bytes(64)) if any(o is None for o in objs) else ref.sig_agg(row[1], objs))
    return _one(got, row[0])


def module_rows(ref):
    """(key aggregation, tweak, nonce, signature) rows of the module's BIP-327 data"""
    from tests import musig_ref as M
    from tests import musig_agg_ref as A
    text = open(os.path.join(REF, "src", "modules", "musig", "vectors.h")).read()
    K, T, Nn, S = [], [], [], []

    def krow(name, keys33):
        pts = [M.parse33(k) for k in keys33]
        return A.make_krow(name, None if M.BAD in pts else pts, keys33=b"".join(keys33))

    pubkeys, tweaks, valid, error = c_initializer(text, "musig_key_agg_vector")
    pubkeys = [bytes(k) for k in pubkeys]; tweaks = [bytes(t) for t in tweaks]
    for i, (kil, ki, expected) in enumerate(valid):
        K.append(krow("BIP-327 key_agg valid %d" % i, [pubkeys[k] for k in ki[:kil]]))
        assert K[-1][4] == 1 and K[-1][6][:32][::-1] == bytes(expected), "BIP-327 key_agg valid %d" % i
    for i, (kil, ki, til, ti, xo, err) in enumerate(error):
        K.append(krow("BIP-327 key_agg error %d (%s)" % (i, err), [pubkeys[k] for k in ki[:kil]]))
        if til:
            assert K[-1][4] == 1
            T.append(A.make_trow("BIP-327 key_agg error %d (%s)" % (i, err), K[-1][5], tweaks[ti[0]], xo[0]))
            assert T[-1][4] == 0
        else:
            assert K[-1][4] == 0
    pnonces, valid, error = c_initializer(text, "musig_nonce_agg_vector")
    pnonces = [bytes(p) for p in pnonces]
    for kind, cases in (("valid", valid), ("error", error)):
        for i, (idx, expected, _) in enumerate(cases):
            ser = pnonces[idx[0]] + pnonces[idx[1]]
            Rs = [(M.parse33(x[:33]), M.parse33(x[33:])) for x in A.split(ser, 66)]
            Nn.append(A.make_nrow("BIP-327 nonce_agg %s %d" % (kind, i), None if any(M.BAD in r for r in Rs) else Rs, ser=ser))
            assert (Nn[-1][3], Nn[-1][4]) == ((1, bytes(expected)) if kind == "valid" else (0, bytes(66))), Nn[-1][0]
    sk, secnonce, aggnonce, msg, pubkeys, pubnonces, tweaks, valid, error = c_initializer(text, "musig_tweak_vector")
    pubkeys = [bytes(k) for k in pubkeys]; tweaks = [bytes(t) for t in tweaks]
    for kind, cases in (("valid", valid), ("error", error)):
        for i, (kil, ki, nil, ni, til, ti, xo, si, expected) in enumerate(cases):
            cache = M.pubkey_agg([M.parse33(pubkeys[k]) for k in ki[:kil]])
            for j, (t, x) in enumerate(zip(ti[:til], xo[:til])):
                T.append(A.make_trow("BIP-327 tweak %s %d, step %d" % (kind, i, j), cache, tweaks[t], x))
                assert T[-1][4] == (1 if kind == "valid" else 0)
                cache = T[-1][5]
    pubkeys, tweaks, psigs, msg, valid, error = c_initializer(text, "musig_sig_agg_vector")
    pubkeys = [bytes(k) for k in pubkeys]; tweaks = [bytes(t) for t in tweaks]; psigs = [bytes(p) for p in psigs]; msg = bytes(msg)
    for kind, cases in (("valid", valid), ("error", error)):
        for i, (kil, ki, til, ti, xo, aggnonce, pil, pi, expected, _) in enumerate(cases):
            cache = ref.pubkey_agg([pubkeys[k] for k in ki[:kil]])
            for t, x in zip(ti[:til], xo[:til]):
                cache = ref.tweak(cache, tweaks[t], x)
            v, session = ref.process(ref.aggnonce(bytes(aggnonce)), msg, cache, None)
            assert v == 1
            ser = b"".join(psigs[k] for k in pi[:pil])
            vals = [M._int(x) for x in A.split(ser, 32)]
            S.append(A.make_srow("BIP-327 sig_agg %s %d" % (kind, i), session, None if any(v >= M.N for v in vals) else vals, ser=ser))
            assert (S[-1][4], S[-1][5]) == ((1, bytes(expected)) if kind == "valid" else (0, bytes(64))), S[-1][0]
    return K, T, Nn, S


def list_midstate():
    """the constant of secp256k1_musig_keyagglist_sha256, read as data"""
    text = open(os.path.join(REF, "src", "modules", "musig", "keyagg_impl.h")).read()
    body = text[text.index("secp256k1_musig_keyagglist_sha256"):]
    words = re.findall(r"0x([0-9a-fA-F]{8})ul", body[:body.index("}")])
    assert len(words) == 8
    return [w.lower() for w in words]


def main():
    from tests import musig_agg_ref as A
    ref = MusigAggRef()
    try:
        mod = module_rows(ref)
        edges = (A.keyagg_edges(), A.tweak_edges(), A.nonce_edges(), A.sig_edges())
        rnd = A.random_rows(64, A.FIXTURE_SEED)
        names = ("keyagg", "tweak", "nonce_agg", "sig_agg")
        n_in = (A.KEYAGG_INPUTS, A.TWEAK_INPUTS, A.NONCE_INPUTS, A.SIG_INPUTS)
        asks = (ask_keyagg, ask_tweak, ask_nonce, ask_sig)
        rows = [list(mod[w]) + list(edges[w]) + list(rnd[w]) for w in range(4)]
        for w in range(4):
            assert len({r[0] for r in rows[w]}) == len(rows[w]), "row names must be unique"
            for row in rows[w]:
                got = asks[w](ref, row)
                assert tuple(got) == tuple(row[1 + n_in[w]:]), "the model disagrees with the reference on %s row %r" % (names[w], row[0])
            assert A.from_json(A.to_json(rows[w], w, n_in[w]), w, n_in[w]) == rows[w]
        assert ref.illegal > 0
        fields = (["name", "keys33", "keys64", "keys65", "verdict", "cache197", "agg_pk64"], ["name", "cache197", "tweak32", "xonly_byte", "verdict", "cache_out197", "pubkey_out64"],
                  ["name", "pubnonces66", "pubnonces132", "verdict", "aggnonce66", "aggnonce132"], ["name", "session133", "sigs32", "sigs36", "verdict", "sig64"])
        out = os.path.join(HERE, "musig_agg_vectors.json")
        with open(out, "w") as f:
            f.write('{"source": "src/modules/musig/vectors.h + tests/musig_agg_ref.py edge lists + random_rows(64, %d); answers: secp256k1_musig_pubkey_agg, _pubkey_ec_tweak_add, '
                    '_pubkey_xonly_tweak_add, _nonce_agg and _partial_sig_agg of the reference",\n' % A.FIXTURE_SEED)
            f.write(' "rebuilt_rows": "name, verdict, sha256 over the inputs as tests/musig_agg_ref.py builds them, the verdict byte and the output fields (each as 4-byte length | bytes, ff for a missing one)",\n')
            f.write(' "keyagg_list_midstate": %s,\n' % json.dumps(list_midstate()))
            for w in range(4):
                f.write(' "%s_fields": %s,\n' % (names[w], json.dumps(fields[w])))
                f.write(' "%s": [\n' % names[w] + ",\n".join("  " + json.dumps(r) for r in A.to_json(rows[w], w, n_in[w])) + "\n ]" + (",\n" if w < 3 else "}\n"))
        print(out, "; ".join("%s: %d rows, %d served" % (names[w], len(rows[w]), sum(r[1 + n_in[w]] for r in rows[w])) for w in range(4)), ";", ref.illegal,
              "illegal-argument callbacks;", os.path.getsize(out), "bytes")
        if "--time" in sys.argv:
            from tests import musig_ref as M
            import numpy as np
            rng = np.random.default_rng(1)
            objs = [M.pt_obj(M.g_mul(M._rand_scalar(rng))) for _ in range(256)]

            def per_call(fn, reps):
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                return (time.perf_counter() - t0) / reps * 1e6
            for m in (2, 16, 256):
                bufs, arr = ref._ptrs(objs[:m], 64)
                cache, agg = ctypes.create_string_buffer(197), ctypes.create_string_buffer(64)
                us = per_call(lambda: ref.lib.secp256k1_musig_pubkey_agg(ref.ctx, agg, cache, arr, m), 2000 // m + 5)
                print("reference, one core (ctypes call overhead included): secp256k1_musig_pubkey_agg of %d keys %.1f us per call, %.2f us per key" % (m, us, us / m))
            c = ctypes.create_string_buffer(cache.raw, 197); t = bytes(M.b32(12345))
            print("  secp256k1_musig_pubkey_xonly_tweak_add %.1f us per call" % per_call(lambda: ref.lib.secp256k1_musig_pubkey_xonly_tweak_add(ref.ctx, None, c, t), 2000))
            for m in (2, 16):
                nb, narr = ref._ptrs([M.pubnonce_obj(M.obj_pt(objs[i]), M.obj_pt(objs[i + 1])) for i in range(m)], 132)
                o = ctypes.create_string_buffer(132)
                print("  secp256k1_musig_nonce_agg of %d pubnonces %.1f us per call" % (m, per_call(lambda: ref.lib.secp256k1_musig_nonce_agg(ref.ctx, o, narr, m), 2000)))
            sess = next(r for r in rows[3] if r[4] == 1 and r[3] is not None)
            sb, sarr = ref._ptrs(A.split(sess[3], 36), 36)
            o = ctypes.create_string_buffer(64)
            print("  secp256k1_musig_partial_sig_agg of %d shares %.2f us per call" % (len(sb), per_call(lambda: ref.lib.secp256k1_musig_partial_sig_agg(ref.ctx, o, sess[1], sarr, len(sb)), 20000)))
    finally:
        ref.close()


if __name__ == "__main__":
    main()
