#!/usr/bin/env python3
"""Writes tests/golden/musig_vectors.json: recorded inputs of secp256k1_musig_partial_sig_verify and secp256k1_musig_nonce_process with
the verdicts and the 133-byte sessions the reference's own functions returned when the file was written.

Run once in the build container:   python tests/golden/make_musig_golden.py [--time]
The reference library the other oracles use is built without the musig module, so this script compiles the unmodified reference with
the musig, extrakeys and schnorrsig modules switched on into a temporary directory outside the repository, loads it with ctypes, asks
it for every verdict and every session and removes the directory again: nothing compiled from the reference is kept, and no test
compiles anything.

Contents: the module's own BIP-327 data (the valid, verify-fail and verify-error cases of the sign/verify vector and the valid cases of
the tweak vector, read from src/modules/musig/vectors.h as data when this script runs and driven through the reference's public
functions: pubkey_agg, the cache tweaks, nonce_agg, the parsers, nonce_process), the edge lists of tests/musig_ref.py and 64 seeded
random items of which every fourth carries one flipped bit.  Serialised inputs go through the reference's parsers (an input that does
not parse gives 0); objects are handed over as they are, with an illegal-argument callback installed that does nothing, so that a wrong
magic or an all-zero key object returns 0 as the engine's contract has it.  The model of tests/musig_ref.py must agree with the
reference on every row, in verdict and in every session byte, and the object layouts it writes must be the parsers', or nothing is
written.  The module's rows are recorded in full; a row tests/musig_ref.py builds again from its seeds is recorded as its name, the
SHA-256 of its inputs and the reference's answers (tests/musig_ref.py: to_json, from_json).  --time also prints the reference's time per call on one core of this machine."""
import ast
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("S2K_REFERENCE", "/root/reference")
REFDEFS = ["-DECMULT_WINDOW_SIZE=15", "-DCOMB_BLOCKS=43", "-DCOMB_TEETH=6", "-DENABLE_MODULE_MUSIG=1", "-DENABLE_MODULE_EXTRAKEYS=1", "-DENABLE_MODULE_SCHNORRSIG=1",
           "-DUSE_ASM_X86_64=1"]
CALLBACK = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_void_p)


class MusigRef:
    """the reference with the module enabled, in a directory that lives as long as this object"""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="s2k_musig_ref_")
        so = os.path.join(self.dir, "libref_musig.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-I" + REF + "/src", "-I" + REF + "/include", "-I" + REF] + REFDEFS +
                              ["-o", so, REF + "/src/secp256k1.c", REF + "/src/precomputed_ecmult.c", REF + "/src/precomputed_ecmult_gen.c"])
        L = self.lib = ctypes.CDLL(so)
        vp, cp, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
        L.secp256k1_context_create.restype = vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        L.secp256k1_context_set_illegal_callback.argtypes = [vp, CALLBACK, vp]
        L.secp256k1_ec_pubkey_parse.argtypes = [vp, vp, cp, sz]
        L.secp256k1_musig_pubkey_agg.argtypes = [vp, vp, vp, vp, sz]
        L.secp256k1_musig_pubkey_ec_tweak_add.argtypes = [vp, vp, vp, cp]
        L.secp256k1_musig_pubkey_xonly_tweak_add.argtypes = [vp, vp, vp, cp]
        L.secp256k1_musig_pubnonce_parse.argtypes = [vp, vp, cp]
        L.secp256k1_musig_aggnonce_parse.argtypes = [vp, vp, cp]
        L.secp256k1_musig_partial_sig_parse.argtypes = [vp, vp, cp]
        L.secp256k1_musig_nonce_agg.argtypes = [vp, vp, vp, sz]
        L.secp256k1_musig_nonce_process.argtypes = [vp, vp, cp, cp, cp, cp]
        L.secp256k1_musig_partial_sig_verify.argtypes = [vp, cp, cp, cp, cp, cp]
        self.ctx = L.secp256k1_context_create(1)
        assert self.ctx
        self.illegal = 0

        def on_illegal(msg, data):
            self.illegal += 1
        self._cb = CALLBACK(on_illegal)                          # (kept alive with the object)
        L.secp256k1_context_set_illegal_callback(self.ctx, self._cb, None)

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def _parse(self, fn, size, data, *more):
        o = ctypes.create_string_buffer(size)
        return o.raw if fn(self.ctx, o, bytes(data), *more) == 1 else None

    def key(self, key33):
        return self._parse(self.lib.secp256k1_ec_pubkey_parse, 64, key33, 33)

    def pubnonce(self, in66):
        return self._parse(self.lib.secp256k1_musig_pubnonce_parse, 132, in66)

    def aggnonce(self, in66):
        return self._parse(self.lib.secp256k1_musig_aggnonce_parse, 132, in66)

    def sig(self, in32):
        return self._parse(self.lib.secp256k1_musig_partial_sig_parse, 36, in32)

    def pubkey_agg(self, keys33):
        objs = [ctypes.create_string_buffer(self.key(k), 64) for k in keys33]
        arr = (ctypes.c_void_p * len(objs))(*[ctypes.addressof(o) for o in objs])
        cache = ctypes.create_string_buffer(197)
        assert self.lib.secp256k1_musig_pubkey_agg(self.ctx, None, cache, arr, len(objs)) == 1
        return cache.raw

    def tweak(self, cache, tweak32, xonly):
        c = ctypes.create_string_buffer(bytes(cache), 197)
        fn = self.lib.secp256k1_musig_pubkey_xonly_tweak_add if xonly else self.lib.secp256k1_musig_pubkey_ec_tweak_add
        return c.raw if fn(self.ctx, None, c, bytes(tweak32)) == 1 else None

    def nonce_agg(self, pubnonce_objs):
        objs = [ctypes.create_string_buffer(o, 132) for o in pubnonce_objs]
        arr = (ctypes.c_void_p * len(objs))(*[ctypes.addressof(o) for o in objs])
        out = ctypes.create_string_buffer(132)
        assert self.lib.secp256k1_musig_nonce_agg(self.ctx, out, arr, len(objs)) == 1
        return out.raw

    def process(self, aggnonce_obj, msg32, cache, adaptor):
        """(verdict, session): the session buffer starts as zeros, which is what the engine documents where the reference writes nothing"""
        out = ctypes.create_string_buffer(133)
        v = self.lib.secp256k1_musig_nonce_process(self.ctx, out, bytes(aggnonce_obj), bytes(msg32), bytes(cache), None if adaptor is None else bytes(adaptor))
        return v, (out.raw if v == 1 else bytes(133))

    def verify(self, sig_obj, pubnonce_obj, key_obj, cache, session):
        return self.lib.secp256k1_musig_partial_sig_verify(self.ctx, bytes(sig_obj), bytes(pubnonce_obj), bytes(key_obj), bytes(cache), bytes(session))


def c_initializer(text, name):
    """the brace initialiser of `name` in a C file as nested Python lists (enumerators as strings)"""
    at = text.index(name + " = {") + len(name) + 3
    depth, end = 0, at
    for end in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[end], 0)
        if depth == 0:
            break
    body = re.sub(r"/\*.*?\*/", "", text[at:end + 1], flags=re.S)
    body = re.sub(r"\b(MUSIG_\w+)\b", r'"\1"', body).replace("{", "[").replace("}", "]")
    return ast.literal_eval(body)


def module_rows(ref):
    """(verify rows, process rows) of the module's BIP-327 data, every object made by the reference's own functions"""
    from tests import musig_ref as M
    text = open(os.path.join(REF, "src", "modules", "musig", "vectors.h")).read()
    V, Pr = [], []

    def vrow(name, sig32, nonce66, key33, cache, session):
        return M.make_vrow(name, cache, session, sig_ser=bytes(sig32), sig_o=ref.sig(sig32), nonce_ser=bytes(nonce66), nonce_o=ref.pubnonce(nonce66),
                           pk_ser=bytes(key33), pk_o=ref.key(key33))

    def session_of(name, agg66, agg_obj, msg, cache):
        Pr.append(M.make_prow(name, msg, cache, nonce_ser=agg66, nonce_o=agg_obj))
        v, sess = ref.process(agg_obj, msg, cache, None)
        assert v == 1
        return sess

    sk, pubkeys, secnonces, pubnonces, aggnonces, msgs, valid, sign_err, vfail, verr = c_initializer(text, "musig_sign_verify_vector")
    pubkeys = [bytes(k) for k in pubkeys]; pubnonces = [bytes(p[:66]) for p in pubnonces]; aggnonces = [bytes(a) for a in aggnonces]; msgs = [bytes(m) for m in msgs]
    for i, (kil, ki, ai, mi, si, expected) in enumerate(valid):
        cache = ref.pubkey_agg([pubkeys[k] for k in ki[:kil]])
        assert cache == M.pubkey_agg([M.parse33(pubkeys[k]) for k in ki[:kil]]), "pubkey_agg of the model"
        sess = session_of("BIP-327 sign/verify valid %d" % i, aggnonces[ai], ref.aggnonce(aggnonces[ai]), msgs[mi], cache)
        V.append(vrow("BIP-327 sign/verify valid %d" % i, expected, pubnonces[0], pubkeys[0], cache, sess))
    for i, (sig, kil, ki, nil, ni, mi, si, err) in enumerate(vfail):
        cache = ref.pubkey_agg([pubkeys[k] for k in ki[:kil]])
        agg = ref.nonce_agg([ref.pubnonce(pubnonces[k]) for k in ni[:nil]])
        R = M.nonce_agg([(M.parse33(pubnonces[k][:33]), M.parse33(pubnonces[k][33:])) for k in ni[:nil]])
        assert agg == M.aggnonce_obj(*R), "nonce_agg of the model"
        sess = session_of("BIP-327 verify fail %d" % i, M.aggnonce_ser(*R), agg, msgs[mi], cache)
        V.append(vrow("BIP-327 verify fail %d (%s)" % (i, err), sig, pubnonces[ni[0]], pubkeys[si], cache, sess))
    cache = ref.pubkey_agg(pubkeys[:3])
    sess = ref.process(ref.aggnonce(aggnonces[0]), msgs[0], cache, None)[1]
    for i, (sig, kil, ki, nil, ni, mi, si, err) in enumerate(verr):
        # the vector ends where a parser refuses; as a row: the refused pubnonce, or the refused key as the signer's, under the valid session
        V.append(vrow("BIP-327 verify error %d (%s)" % (i, err), sig, pubnonces[ni[si]], pubkeys[ki[si]], cache, sess))
    sk, secnonce, aggnonce, msg, pubkeys, pubnonces, tweaks, valid, error = c_initializer(text, "musig_tweak_vector")
    pubkeys = [bytes(k) for k in pubkeys]; pubnonces = [bytes(p[:66]) for p in pubnonces]; tweaks = [bytes(t) for t in tweaks]; aggnonce = bytes(aggnonce); msg = bytes(msg)
    for i, (kil, ki, nil, ni, til, ti, xo, si, expected) in enumerate(valid):
        cache = ref.pubkey_agg([pubkeys[k] for k in ki[:kil]])
        mc = M.pubkey_agg([M.parse33(pubkeys[k]) for k in ki[:kil]])
        for t, x in zip(ti[:til], xo[:til]):
            cache, mc = ref.tweak(cache, tweaks[t], x), M.tweak_add(mc, tweaks[t], x)
        assert cache is not None and cache == mc, "the cache tweaks of the model"
        sess = session_of("BIP-327 tweak valid %d" % i, aggnonce, ref.aggnonce(aggnonce), msg, cache)
        V.append(vrow("BIP-327 tweak valid %d" % i, expected, pubnonces[ni[si]], pubkeys[0], cache, sess))
    return V, Pr


def ask_verify(ref, row):
    """the reference's answer to a verify row: objects as they are, serialised fields through its parsers"""
    from tests import musig_ref as M
    name, sig_ser, sig_o, nonce_ser, nonce_o, pk_ser, pk_o, cache, session, _ = row
    for ser, obj, parse in ((sig_ser, sig_o, ref.sig), (nonce_ser, nonce_o, ref.pubnonce), (pk_ser, pk_o, ref.key)):
        if ser is not None and obj is not None:
            assert parse(ser) == obj, "the object layout of the model: " + name
        if obj is None:
            assert ser is not None and parse(ser) is None, name + ": a row without an object whose serialisation parses"
    objs = [obj if obj is not None else parse(ser) for ser, obj, parse in ((sig_ser, sig_o, ref.sig), (nonce_ser, nonce_o, ref.pubnonce), (pk_ser, pk_o, ref.key))]
    if any(o is None for o in objs):
        return 0
    return ref.verify(objs[0], objs[1], objs[2], cache, session)


def ask_process(ref, row):
    name, nonce_ser, nonce_o, msg, cache, adaptor, _, _ = row
    if nonce_ser is not None and nonce_o is not None:
        assert ref.aggnonce(nonce_ser) == nonce_o, "the object layout of the model: " + name
    obj = nonce_o if nonce_o is not None else ref.aggnonce(nonce_ser)
    if obj is None:
        return 0, bytes(133)
    return ref.process(obj, msg, cache, adaptor)


def main():
    from tests import musig_ref as M
    ref = MusigRef()
    try:
        mv, mp = module_rows(ref)
        ev, ep = M.edge_cases()
        rv, rp = M.random_items(64, M.FIXTURE_SEED)
        V, Pr = mv + ev + rv, mp + ep + rp
        for row in V:
            v = ask_verify(ref, row)
            assert v == row[9], "the model disagrees with the reference on verify row %r: %d vs %d" % (row[0], row[9], v)
        for row in Pr:
            v, sess = ask_process(ref, row)
            assert (v, sess) == (row[6], row[7]), "the model disagrees with the reference on process row %r" % row[0]
        names = {r[0]: r[9] for r in mv}
        assert all(names["BIP-327 sign/verify valid %d" % i] == 1 for i in range(4)) and all(names["BIP-327 tweak valid %d" % i] == 1 for i in range(5))
        assert sum(names.values()) == 9 and ref.illegal > 0
        assert M.from_json(M.to_json(V, M.VERIFY_INPUTS), M.VERIFY_INPUTS) == V and M.from_json(M.to_json(Pr, M.PROCESS_INPUTS), M.PROCESS_INPUTS) == Pr
        out = os.path.join(HERE, "musig_vectors.json")
        with open(out, "w") as f:
            f.write('{"source": "src/modules/musig/vectors.h + tests/musig_ref.py edge_cases() + random_items(64, %d); verdicts and sessions: secp256k1_musig_partial_sig_verify and secp256k1_musig_nonce_process of the reference",\n' % M.FIXTURE_SEED)
            f.write(' "verify_fields": ["name", "sig_ser", "sig_obj", "nonce_ser", "nonce_obj", "pk_ser", "pk_obj", "cache", "session", "verdict"],\n')
            f.write(' "rebuilt_rows": "name, sha256 of the inputs as tests/musig_ref.py builds them, then the answers (verdict; for process also session_out)",\n')
            f.write(' "verify": [\n' + ",\n".join("  " + json.dumps(r) for r in M.to_json(V, M.VERIFY_INPUTS)) + "\n ],\n")
            f.write(' "process_fields": ["name", "nonce_ser", "nonce_obj", "msg32", "cache", "adaptor", "verdict", "session_out"],\n')
            f.write(' "process": [\n' + ",\n".join("  " + json.dumps(r) for r in M.to_json(Pr, M.PROCESS_INPUTS)) + "\n ]}\n")
        print(out, len(V), "verify rows,", sum(r[9] for r in V), "valid;", len(Pr), "process rows,", sum(r[6] for r in Pr), "served;", ref.illegal,
              "illegal-argument callbacks;", os.path.getsize(out), "bytes")
        for f in M.ALL_VERIFY_FORMATS:
            print("  formats", f, "run", sum(1 for r in V if M.verify_formats(r, *f) is not None), "of", len(V))
        if "--time" in sys.argv:
            vv = [r for r in V if r[9] == 1 and None not in r[1:7]]
            pp = [r for r in Pr if r[6] == 1 and r[2] is not None]
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                for r in vv:
                    ref.lib.secp256k1_musig_partial_sig_verify(ref.ctx, r[2], r[4], r[6], r[7], r[8])
            dv = (time.perf_counter() - t0) / (reps * len(vv))
            out133 = ctypes.create_string_buffer(133)
            t0 = time.perf_counter()
            for _ in range(reps):
                for r in pp:
                    ref.lib.secp256k1_musig_nonce_process(ref.ctx, out133, r[2], r[3], r[4], r[5])
            dp = (time.perf_counter() - t0) / (reps * len(pp))
            print("reference, one core, valid items (ctypes call overhead included): secp256k1_musig_partial_sig_verify %.1f us per call, "
                  "secp256k1_musig_nonce_process %.1f us per call" % (dv * 1e6, dp * 1e6))
    finally:
        ref.close()


if __name__ == "__main__":
    main()
