#!/usr/bin/env python3
"""Writes tests/golden/s2c_vectors.json: recorded inputs of secp256k1_ecdsa_s2c_verify_commit and secp256k1_anti_exfil_host_verify with the
two verdicts the reference's own functions returned when the file was written, and recorded outputs of
secp256k1_ecdsa_anti_exfil_host_commit.

Run once in the build container:   python tests/golden/make_s2c_golden.py [--time]
The reference library the other oracles use is built without the ecdsa_s2c module, so this script compiles the unmodified reference with
the module switched on into a temporary directory outside the repository, loads it with ctypes, asks it for every verdict and removes the
directory again: nothing compiled from the reference is kept, and no test compiles anything.

Contents: the module's two fixed vectors (key, message, data and expected openings read from the module's test file as data when this
script runs; the signatures are the reference's own secp256k1_ecdsa_s2c_sign, and the serialised openings are asserted to be the
expected ones), the same two through the anti-exfil flow (host_commit -> signer_commit -> anti_exfil_sign -> host_verify), the edge list
of tests/s2c_ref.py and 64 seeded random items of which every fourth carries one flipped bit.  Every verdict is the reference's, except
on the objects no caller of the reference can hold (all-zero key and opening objects, signature objects with limbs >= n: they carry the
engine's contract).  The model of tests/s2c_ref.py must agree with every verdict the reference gave, or nothing is written.
--time also prints the reference's time per call on one core of this machine."""
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
REFDEFS = ["-DECMULT_WINDOW_SIZE=15", "-DCOMB_BLOCKS=43", "-DCOMB_TEETH=6", "-DENABLE_MODULE_ECDSA_S2C=1", "-DUSE_ASM_X86_64=1"]
RANDOM_SEED = 5602


class S2cRef:
    """the reference with the module enabled, in a directory that lives as long as this object"""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="s2k_s2c_ref_")
        so = os.path.join(self.dir, "libref_s2c.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-I" + REF + "/src", "-I" + REF + "/include", "-I" + REF] + REFDEFS +
                              ["-o", so, REF + "/src/secp256k1.c", REF + "/src/precomputed_ecmult.c", REF + "/src/precomputed_ecmult_gen.c"])
        L = self.lib = ctypes.CDLL(so)
        vp, cp = ctypes.c_void_p, ctypes.c_char_p
        L.secp256k1_context_create.restype = vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        for name, args in {"secp256k1_ec_pubkey_parse": [vp, vp, cp, ctypes.c_size_t], "secp256k1_ec_pubkey_create": [vp, vp, cp],
                           "secp256k1_ecdsa_signature_parse_compact": [vp, vp, cp], "secp256k1_ecdsa_signature_parse_der": [vp, vp, cp, ctypes.c_size_t],
                           "secp256k1_ecdsa_signature_serialize_compact": [vp, vp, vp],
                           "secp256k1_ecdsa_s2c_opening_parse": [vp, vp, cp], "secp256k1_ecdsa_s2c_opening_serialize": [vp, vp, vp],
                           "secp256k1_ecdsa_s2c_sign": [vp, vp, vp, cp, cp, cp], "secp256k1_ecdsa_s2c_verify_commit": [vp, vp, cp, vp],
                           "secp256k1_ecdsa_anti_exfil_host_commit": [vp, vp, cp], "secp256k1_ecdsa_anti_exfil_signer_commit": [vp, vp, cp, cp, cp],
                           "secp256k1_anti_exfil_sign": [vp, vp, cp, cp, cp], "secp256k1_anti_exfil_host_verify": [vp, vp, cp, vp, cp, vp]}.items():
            f = getattr(L, name); f.restype = ctypes.c_int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(1)
        assert self.ctx

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def _obj(self, fn, *args):
        o = ctypes.create_string_buffer(64)
        return o if fn(self.ctx, o, *args) == 1 else None

    def pubkey(self, key33):
        return self._obj(self.lib.secp256k1_ec_pubkey_parse, bytes(key33), len(key33))

    def opening(self, op33):
        return self._obj(self.lib.secp256k1_ecdsa_s2c_opening_parse, bytes(op33)) if len(op33) == 33 else None

    def sig(self, sig, der):
        return self._obj(self.lib.secp256k1_ecdsa_signature_parse_der, bytes(sig), len(sig)) if der else self._obj(self.lib.secp256k1_ecdsa_signature_parse_compact, bytes(sig))

    def verdicts(self, sig, der, msg32, pubkey33, data32, opening33):
        """what a caller of the reference gets: an object that does not parse never reaches the verifier"""
        so, po, oo = self.sig(sig, der), self.pubkey(pubkey33), self.opening(opening33)
        c = 0 if so is None or oo is None else self.lib.secp256k1_ecdsa_s2c_verify_commit(self.ctx, so, bytes(data32), oo)
        h = 0 if so is None or oo is None or po is None else self.lib.secp256k1_anti_exfil_host_verify(self.ctx, so, bytes(msg32), po, bytes(data32), oo)
        return c, h

    def host_commit(self, rand32):
        o = ctypes.create_string_buffer(32)
        assert self.lib.secp256k1_ecdsa_anti_exfil_host_commit(self.ctx, o, bytes(rand32)) == 1
        return o.raw

    def compact(self, sigobj):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ecdsa_signature_serialize_compact(self.ctx, o, sigobj) == 1
        return o.raw

    def ser_opening(self, obj):
        o = ctypes.create_string_buffer(33)
        assert self.lib.secp256k1_ecdsa_s2c_opening_serialize(self.ctx, o, obj) == 1
        return o.raw


def module_vectors(ref):
    """the module's fixed vectors as items: the s2c signature of each, then each through the anti-exfil flow"""
    from tests import s2c_ref as S
    text = open(os.path.join(REF, "src", "modules", "ecdsa_s2c", "tests_impl.h")).read()

    def hexes(block):
        return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", block))
    table = text[text.index("static ecdsa_s2c_test ecdsa_s2c_tests[] = {"):text.index("static void test_ecdsa_s2c_fixed_vectors(void)")]
    rows = [hexes(m.group(0)) for m in re.finditer(r"\{\s*\{[^{}]*\},\s*\{[^{}]*\},\s*\{[^{}]*\},\s*\}", table)]
    assert len(rows) == 2 and all(len(r) == 32 + 33 + 33 for r in rows)
    fn = text[text.index("static void test_ecdsa_s2c_fixed_vectors(void)"):text.index("static void test_ecdsa_s2c_sign_verify(void)")]
    arr = {m.group(1): hexes(m.group(2)) for m in re.finditer(r"const unsigned char (\w+)\[32\] = \{(.*?)\};", fn, re.S)}
    key, msg = arr["privkey"], arr["message"]
    pko = ctypes.create_string_buffer(64)
    assert ref.lib.secp256k1_ec_pubkey_create(ref.ctx, pko, key) == 1
    pk33 = S.ser33(S.pt_mul(int.from_bytes(key, "big"), S.G))
    assert ref.pubkey(pk33).raw == pko.raw
    out = []
    for i, row in enumerate(rows):
        data, want_op, want_exfil = row[:32], row[32:65], row[65:]
        so, oo = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        assert ref.lib.secp256k1_ecdsa_s2c_sign(ref.ctx, so, oo, msg, key, data) == 1
        assert ref.ser_opening(oo) == want_op, "vector %d: the opening is not expected_s2c_opening" % i
        out.append(S.make_item("module vector %d" % i, ref.compact(so), msg, pk33, data, want_op))
        eo = ctypes.create_string_buffer(64)
        assert ref.lib.secp256k1_ecdsa_anti_exfil_signer_commit(ref.ctx, eo, msg, key, data) == 1
        assert ref.ser_opening(eo) == want_exfil, "vector %d: the opening is not expected_s2c_exfil_opening" % i
        # the flow with the vector's data as the host's randomness: the signer commits to the host's commitment, signs, the host verifies
        fo, fs = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        assert ref.lib.secp256k1_ecdsa_anti_exfil_signer_commit(ref.ctx, fo, msg, key, ref.host_commit(data)) == 1
        assert ref.lib.secp256k1_anti_exfil_sign(ref.ctx, fs, msg, key, data) == 1
        assert ref.lib.secp256k1_anti_exfil_host_verify(ref.ctx, fs, msg, pko, data, fo) == 1
        out.append(S.make_item("module vector %d anti-exfil" % i, ref.compact(fs), msg, pk33, data, ref.ser_opening(fo)))
        # and with the commitment the module's own test hands the signer: that opening does not belong to a signature over `data`
        out.append(S.make_item("module vector %d with the exfil opening" % i, ref.compact(fs), msg, pk33, data, want_exfil))
    return out


def main():
    from tests import s2c_ref as S
    ref = S2cRef()
    try:
        items = module_vectors(ref) + S.edge_cases() + S.random_items(64, RANDOM_SEED)
        rows, asked = [], 0
        for it in items:
            name, sig, msg, pk, data, op, c, h, only = it
            if only in (None, "der"):
                v = ref.verdicts(sig, only == "der", msg, pk, data, op); asked += 1
                assert v == (c, h), "the model disagrees with the reference on %r: %r vs %r" % (name, (c, h), v)
                for key in (pk, op):                      # the object layout s2c_ref.key_object writes is the reference's
                    o = ref.pubkey(key)
                    assert (o.raw if o else None) == S.key_object(key), name
                o = None if only == "der" else ref.sig(sig, False)
                assert only == "der" or (o.raw if o else None) == S.sig_object(sig), name
            rows.append(it)
        assert [(r[6], r[7]) for r in rows[:6]] == [(1, 1), (1, 1), (0, 0)] * 2
        commits = [(it[4], ref.host_commit(it[4])) for it in rows[:8]] + [(bytes(32), ref.host_commit(bytes(32))), (b"\xff" * 32, ref.host_commit(b"\xff" * 32))]
        for rnd, cm in commits:
            assert S.host_commit(rnd) == cm
        out = os.path.join(HERE, "s2c_vectors.json")
        with open(out, "w") as f:
            f.write('{"source": "the module\'s own vectors + tests/s2c_ref.py edge_cases() + random_items(64, %d); verdicts: secp256k1_ecdsa_s2c_verify_commit and '
                    'secp256k1_anti_exfil_host_verify of the reference",\n' % RANDOM_SEED)
            f.write(' "fields": ["name", "sig", "msg32", "pubkey", "data32", "opening", "commit", "host", "fmt_only"],\n')
            f.write(' "host_commit": [\n' + ",\n".join("  " + json.dumps([a.hex(), b.hex()]) for a, b in commits) + "\n ],\n")
            f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps(r) for r in S.to_json(rows)) + "\n ]}\n")
        print(out, len(rows), "vectors,", asked, "asked of the reference,", sum(r[6] for r in rows), "commit,", sum(r[7] for r in rows), "host,", os.path.getsize(out), "bytes")
        if "--time" in sys.argv:
            valid = [r for r in rows if r[7] == 1 and r[8] is None]
            objs = [(ref.sig(r[1], False), r[2], ref.pubkey(r[3]), r[4], ref.opening(r[5])) for r in valid]
            reps = 20
            for what, call in (("secp256k1_ecdsa_s2c_verify_commit", lambda s, m, p, d, o: ref.lib.secp256k1_ecdsa_s2c_verify_commit(ref.ctx, s, d, o)),
                               ("secp256k1_anti_exfil_host_verify", lambda s, m, p, d, o: ref.lib.secp256k1_anti_exfil_host_verify(ref.ctx, s, m, p, d, o))):
                t0 = time.perf_counter()
                for _ in range(reps):
                    for a in objs:
                        call(*a)
                dt = (time.perf_counter() - t0) / (reps * len(objs))
                print("reference %s, one core, valid items: %.1f us per call (ctypes call overhead included)" % (what, dt * 1e6))
    finally:
        ref.close()


if __name__ == "__main__":
    main()
