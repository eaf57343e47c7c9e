#!/usr/bin/env python3
"""Writes tests/golden/adaptor_vectors.json: recorded inputs of secp256k1_ecdsa_adaptor_verify with the verdict the reference's own
function returned when the file was written.

Run once in the build container:   python tests/golden/make_adaptor_golden.py [--time]
The reference library the other oracles use is built without the ecdsa_adaptor module, so this script compiles the unmodified reference
with the module switched on into a temporary directory outside the repository, loads it with ctypes, asks it for every verdict and removes
the directory again: nothing compiled from the reference is kept, and no test compiles anything.

Contents: the three verification vectors and the issue-335 vector of the module's own test file (read from it as data when this script
runs), the edge list of tests/adaptor_ref.py and 64 seeded random items of which every fourth carries one flipped bit.  Every verdict is
the reference's, except on the all-zero key objects (engine only: the reference calls its illegal-argument callback there; they carry
the engine's contract, 0).  The model of tests/adaptor_ref.py must agree with every verdict the reference gave, or nothing is written.
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
REFDEFS = ["-DECMULT_WINDOW_SIZE=15", "-DCOMB_BLOCKS=43", "-DCOMB_TEETH=6", "-DENABLE_MODULE_ECDSA_ADAPTOR=1", "-DUSE_ASM_X86_64=1"]
RANDOM_SEED = 5502


class AdaptorRef:
    """the reference with the module enabled, in a directory that lives as long as this object"""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="s2k_adaptor_ref_")
        so = os.path.join(self.dir, "libref_adaptor.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-I" + REF + "/src", "-I" + REF + "/include", "-I" + REF] + REFDEFS +
                              ["-o", so, REF + "/src/secp256k1.c", REF + "/src/precomputed_ecmult.c", REF + "/src/precomputed_ecmult_gen.c"])
        L = self.lib = ctypes.CDLL(so)
        L.secp256k1_context_create.restype = ctypes.c_void_p
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        L.secp256k1_ec_pubkey_parse.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.secp256k1_ecdsa_adaptor_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
        self.ctx = L.secp256k1_context_create(1)
        assert self.ctx

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def parse(self, key33):
        o = ctypes.create_string_buffer(64)
        return o if self.lib.secp256k1_ec_pubkey_parse(self.ctx, o, bytes(key33), 33) == 1 else None

    def verify(self, sig162, pubkey33, msg32, enckey33):
        """what a caller of the reference gets: a key that does not parse never reaches the verifier"""
        pk, ek = self.parse(pubkey33), self.parse(enckey33)
        if pk is None or ek is None:
            return 0
        return self.lib.secp256k1_ecdsa_adaptor_verify(self.ctx, bytes(sig162), pk, bytes(msg32), ek)


def module_vectors():
    """the arrays of the module's test file, as bytes: (name, sig162, pubkey33, msg32, enckey33) of spec vectors 0..2 and of issue 335"""
    from tests import adaptor_ref as A
    text = open(os.path.join(REF, "src", "modules", "ecdsa_adaptor", "tests_impl.h")).read()

    def arrays(block):
        return {m.group(1): bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", m.group(2)))
                for m in re.finditer(r"unsigned char (\w+)\[\d*\] = \{(.*?)\};", block, re.S)}
    out = []
    spec = text[text.index("static void test_ecdsa_adaptor_spec_vectors(void)"):]
    for i in range(3):
        a = arrays(spec[spec.index("/* Test vector %d */" % i):spec.index("/* Test vector %d */" % (i + 1))])
        out.append(("module vector %d" % i, a["adaptor_sig"], a["pubkey"], a["message_hash"], a["encryption_key"]))
    blk = text[text.index("static void adaptor_test_issue335(void)"):]
    a = arrays(blk[:blk.index("secp256k1_pubkey pubkey;")])
    out.append(("module issue 335: R1 at infinity", a["adaptor_sig"], A.ser33(A.pt_mul(int.from_bytes(a["seckey"], "big"), A.G)), a["msg"],
                A.ser33(A.pt_mul(int.from_bytes(a["deckey"], "big"), A.G))))
    return out


def main():
    from tests import adaptor_ref as A
    ref = AdaptorRef()
    try:
        items = [A.make_item(*v) for v in module_vectors()] + A.edge_cases() + A.random_items(64, RANDOM_SEED)
        rows, asked = [], 0
        for it in items:
            name, sig, pk, msg, ek, model, only = it
            if only is None:
                v = ref.verify(sig, pk, msg, ek); asked += 1
                assert v == model, "the model disagrees with the reference on %r: %d vs %d" % (name, model, v)
                for key in (pk, ek):                      # the object layout adaptor_ref.key_object writes is the reference's
                    o = ref.parse(key)
                    assert (o.raw if o else None) == A.key_object(key), name
            else:
                v = 0
            rows.append((name, sig, pk, msg, ek, v, only))
        assert [r[5] for r in rows[:4]] == [1, 1, 0, 0]
        out = os.path.join(HERE, "adaptor_vectors.json")
        with open(out, "w") as f:
            f.write('{"source": "the module\'s own vectors + tests/adaptor_ref.py edge_cases() + random_items(64, %d); verdicts: secp256k1_ecdsa_adaptor_verify of the reference",\n' % RANDOM_SEED)
            f.write(' "fields": ["name", "sig162", "pubkey", "msg32", "enckey", "verdict", "fmt_only"],\n')
            f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps(r) for r in A.to_json(rows)) + "\n ]}\n")
        print(out, len(rows), "vectors,", asked, "asked of the reference,", sum(r[5] for r in rows), "valid,", os.path.getsize(out), "bytes")
        if "--time" in sys.argv:
            valid = [r for r in rows if r[5] == 1 and r[6] is None]
            objs = [(r[1], ref.parse(r[2]), r[3], ref.parse(r[4])) for r in valid]
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                for sig, pk, msg, ek in objs:
                    ref.lib.secp256k1_ecdsa_adaptor_verify(ref.ctx, sig, pk, msg, ek)
            dt = (time.perf_counter() - t0) / (reps * len(objs))
            print("reference secp256k1_ecdsa_adaptor_verify, one core, valid items: %.1f us per call (ctypes call overhead included)" % (dt * 1e6))
    finally:
        ref.close()


if __name__ == "__main__":
    main()
