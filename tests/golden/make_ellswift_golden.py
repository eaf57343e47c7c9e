#!/usr/bin/env python3
"""Writes tests/golden/ellswift_vectors.json: recorded inputs of secp256k1_ellswift_decode and secp256k1_ellswift_encode with what the
reference's own functions returned when the file was written.

Run once in the build container:   python tests/golden/make_ellswift_golden.py [--time]
The reference library the other oracles use is built without the ellswift module, so this script compiles the unmodified reference with
the module switched on into a temporary directory outside the repository, loads it with ctypes, asks it for every answer and removes the
directory again: nothing compiled from the reference is kept, and no test compiles anything.

Contents: the module's own vectors, read from its test file as data when this script runs (the partial-inverse vectors {u, x, bitmap,
encs[8]} and the decode vectors {enc, x, odd_y}); the decode edge list of tests/ellswift_ref.py with the reference's key objects; 64
seeded (key, rnd32) pairs with the reference's ell64, the model's attempt count and successful branch value, each ell64 decoded back by
the reference; and the refused keys.  The model of tests/ellswift_ref.py must agree with every answer the reference gave (and with the
module's vectors, which no public function of the reference reaches directly), or nothing is written.
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
REFDEFS = ["-DECMULT_WINDOW_SIZE=15", "-DCOMB_BLOCKS=43", "-DCOMB_TEETH=6", "-DENABLE_MODULE_ELLSWIFT=1", "-DUSE_ASM_X86_64=1"]


class EllswiftRef:
    """the reference with the module enabled, in a directory that lives as long as this object"""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="s2k_ellswift_ref_")
        so = os.path.join(self.dir, "libref_ellswift.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-I" + REF + "/src", "-I" + REF + "/include", "-I" + REF] + REFDEFS +
                              ["-o", so, REF + "/src/secp256k1.c", REF + "/src/precomputed_ecmult.c", REF + "/src/precomputed_ecmult_gen.c"])
        L = self.lib = ctypes.CDLL(so)
        vp, cp = ctypes.c_void_p, ctypes.c_char_p
        L.secp256k1_context_create.restype = vp
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        for name, args in {"secp256k1_ec_pubkey_parse": [vp, vp, cp, ctypes.c_size_t], "secp256k1_ec_pubkey_serialize": [vp, vp, vp, vp, ctypes.c_uint],
                           "secp256k1_ellswift_decode": [vp, vp, cp], "secp256k1_ellswift_encode": [vp, vp, vp, cp]}.items():
            f = getattr(L, name); f.restype = ctypes.c_int; f.argtypes = args
        self.ctx = L.secp256k1_context_create(1)
        assert self.ctx
        # the all-zero object raises the illegal-argument callback, which aborts by default: count instead
        self.illegal = 0
        CB = ctypes.CFUNCTYPE(None, cp, vp)
        self._cb = CB(self._on_illegal)
        L.secp256k1_context_set_illegal_callback.restype = None
        L.secp256k1_context_set_illegal_callback.argtypes = [vp, CB, vp]
        L.secp256k1_context_set_illegal_callback(self.ctx, self._cb, None)

    def _on_illegal(self, msg, data):
        self.illegal += 1

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def pubkey(self, key33):
        o = ctypes.create_string_buffer(64)
        return o.raw if self.lib.secp256k1_ec_pubkey_parse(self.ctx, o, bytes(key33), len(key33)) == 1 else None

    def ser33(self, obj):
        o = ctypes.create_string_buffer(33); n = ctypes.c_size_t(33)
        assert self.lib.secp256k1_ec_pubkey_serialize(self.ctx, o, ctypes.byref(n), bytes(obj), 0x102) == 1 and n.value == 33
        return o.raw

    def decode(self, ell64):
        o = ctypes.create_string_buffer(64)
        assert self.lib.secp256k1_ellswift_decode(self.ctx, o, bytes(ell64)) == 1
        return o.raw

    def encode(self, obj, rnd32):
        o = ctypes.create_string_buffer(b"\xaa" * 64, 64)
        r = self.lib.secp256k1_ellswift_encode(self.ctx, o, bytes(obj), bytes(rnd32))
        return r, o.raw


def module_vectors():
    """-> (inv, dec): [[u, x, bitmap, [t or 0] * 8]] and [[enc, x, odd_y]] as the module's test file holds them"""
    text = open(os.path.join(REF, "src", "modules", "ellswift", "tests_impl.h")).read()
    fe = r"SECP256K1_FE_CONST\(([^)]*)\)"

    def fe_int(words):
        w = [int(x.strip(), 0) for x in words.split(",")]
        assert len(w) == 8
        v = 0
        for x in w:
            v = (v << 32) | x
        return v
    a = text[text.index("ellswift_xswiftec_inv_tests[] = {"):text.index("ellswift_decode_tests[] = {")]
    inv = []
    for m in re.finditer(r"\{(0x[0-9a-fA-F]{2}), " + fe + ", " + fe + r", \{((?:" + fe + r"(?:, )?){8})\}\}", a):
        encs = [fe_int(w) for w in re.findall(fe, m.group(4))]
        inv.append([fe_int(m.group(2)), fe_int(m.group(3)), int(m.group(1), 16), encs])
    b = text[text.index("ellswift_decode_tests[] = {"):]
    b = b[:b.index("};")]
    dec = []
    for m in re.finditer(r"\{\{([^}]*)\}, " + fe + r", (\d)\}", b):
        enc = bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", m.group(1)))
        assert len(enc) == 64
        dec.append([enc, fe_int(m.group(2)), int(m.group(3))])
    assert len(inv) >= 30 and len(dec) >= 70, (len(inv), len(dec))
    return inv, dec


def main():
    from tests import ellswift_ref as E
    inv, dec = module_vectors()
    ref = EllswiftRef()
    try:
        asked = 0
        # the module's partial-inverse vectors: the model alone (the function is static in the reference)
        for u, x, bitmap, encs in inv:
            for c in range(8):
                t = E.xswiftec_inv(x, u, c)
                assert (t is not None) == bool((bitmap >> c) & 1), "partial inverse: bitmap"
                if t is not None:
                    assert t == encs[c] and E.xswiftec(u, t)[0] == x, "partial inverse: t"
        # the module's decode vectors: model and reference
        dec_rows = []
        for enc, x, odd in dec:
            obj = ref.decode(enc); asked += 1
            mx, my, which = E.decode(enc)
            assert (mx, my & 1) == (x, odd) and obj == E.pubkey_object(mx, my) and ref.ser33(obj) == E.ser33(mx, my), "decode vector"
            dec_rows.append(["module vector", enc.hex(), obj.hex(), which])
        for name, enc in E.decode_edges():
            obj = ref.decode(enc); asked += 1
            mx, my, which = E.decode(enc)
            assert obj == E.pubkey_object(mx, my) and ref.ser33(obj) == E.ser33(mx, my), "the model disagrees with the reference on %r" % name
            dec_rows.append([name, enc.hex(), obj.hex(), which])
        enc_rows, attempts = [], []
        for name, key33, rnd in E.encode_items():
            obj = ref.pubkey(key33)
            r, ell = ref.encode(obj, rnd); asked += 1
            mr, mell, att, c = E.encode(key33, 2, rnd)
            assert (r, ell) == (1, mell) == (mr, mell), "the model disagrees with the reference on %r" % name
            assert E.encode(obj, 1, rnd)[1] == ell
            assert ref.decode(ell) == obj; asked += 1
            enc_rows.append([name, key33.hex(), obj.hex(), rnd.hex(), ell.hex(), att, c])
            attempts.append(att)
        assert set(r[6] for r in enc_rows) == set(range(8)) and min(attempts) == 1 and max(attempts) >= 12
        ref_rows = []
        for name, key, fmt in E.refused_keys():
            if fmt == 2:
                assert ref.pubkey(key) is None, name; asked += 1
            else:
                before = ref.illegal
                r, ell = ref.encode(key, bytes(32)); asked += 1
                assert ref.illegal == before + 1 and r == 0 and ell == bytes(64), name
            assert E.encode(key, fmt, bytes(32))[:2] == (0, bytes(64)), name
            ref_rows.append([name, key.hex(), fmt])
        out = os.path.join(HERE, "ellswift_vectors.json")
        with open(out, "w") as f:
            f.write('{"source": "src/modules/ellswift/tests_impl.h (xswiftec_inv and decode vectors) + tests/ellswift_ref.py decode_edges(), encode_items(), refused_keys(); '
                    'answers: secp256k1_ellswift_decode and secp256k1_ellswift_encode of the reference",\n')
            f.write(' "xswiftec_inv_fields": ["u", "x", "bitmap", "encs"],\n "xswiftec_inv": [\n' +
                    ",\n".join("  " + json.dumps(["%064x" % u, "%064x" % x, bm, ["%064x" % t for t in encs]]) for u, x, bm, encs in inv) + "\n ],\n")
            f.write(' "decode_fields": ["name", "ell64", "pubkey_object", "which"],\n "decode": [\n' + ",\n".join("  " + json.dumps(r) for r in dec_rows) + "\n ],\n")
            f.write(' "encode_fields": ["name", "key33", "pubkey_object", "rnd32", "ell64", "attempts", "branch"],\n "encode": [\n' +
                    ",\n".join("  " + json.dumps(r) for r in enc_rows) + "\n ],\n")
            f.write(' "refused_fields": ["name", "key", "key_format"],\n "refused": [\n' + ",\n".join("  " + json.dumps(r) for r in ref_rows) + "\n ]}\n")
        print(out, len(inv), "partial-inverse vectors,", len(dec_rows), "decode items,", len(enc_rows), "encode items,", len(ref_rows), "refused keys,", asked,
              "asked of the reference,", os.path.getsize(out), "bytes; attempts: mean %.2f, max %d, rounds per wavefront %.1f" %
              (sum(attempts) / len(attempts), max(attempts), E.rounds_per_wavefront(attempts)))
        if "--time" in sys.argv:
            encs = [bytes.fromhex(r[1]) for r in dec_rows]
            pairs = [(bytes.fromhex(r[2]), bytes.fromhex(r[3])) for r in enc_rows]
            reps = 50
            o = ctypes.create_string_buffer(64)
            t0 = time.perf_counter()
            for _ in range(reps):
                for e in encs:
                    ref.lib.secp256k1_ellswift_decode(ref.ctx, o, e)
            print("reference secp256k1_ellswift_decode, one core: %.1f us per call (ctypes call overhead included)" % ((time.perf_counter() - t0) / (reps * len(encs)) * 1e6))
            t0 = time.perf_counter()
            for _ in range(reps):
                for k, r in pairs:
                    ref.lib.secp256k1_ellswift_encode(ref.ctx, o, k, r)
            print("reference secp256k1_ellswift_encode, one core: %.1f us per call (ctypes call overhead included; %.2f attempts per item)" %
                  ((time.perf_counter() - t0) / (reps * len(pairs)) * 1e6, sum(attempts) / len(attempts)))
    finally:
        ref.close()


if __name__ == "__main__":
    main()
