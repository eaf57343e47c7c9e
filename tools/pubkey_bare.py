#!/usr/bin/env python3
"""Device-resident timing of the public-key calls (csrc/engine_pubkey.hip) next to calls that existed before them, in one process, on
the same keys:

    python tools/pubkey_bare.py [--sizes 65536 1048576] [--set-sizes 2 16 256] [--rounds 7] [--ab-lib OTHER.so] [--out profiles/pubkey_rates.json]

    convert 2 -> 1   against secp256k1_generator_parse_batch_dev       (both: one square root per item; the same x, prefix 0a for the generator)
    convert 1 -> 2   against secp256k1_generator_serialize_batch_dev   (both: bytes in, bytes out)
    tweak_mul 1 -> 1 against s2k_ecmult_batch_dev with ng = NULL       (the same multiplication: same keys, same scalars)
    combine          n keys as 2-, 16- and 256-key sets, formats 1 and 2, against secp256k1_musig_nonce_agg_batch_dev over n pubnonce
                     objects in sessions of the same sizes (n points per column, two columns: its time is also given per column)

Times are the HIP events the engine records around a call's launches (s2k_engine_last_ms(0): the whole chain).  After two warm-up
calls of each, the calls alternate for --rounds rounds; every figure is the median of the rounds with their minimum and maximum.

--ab-lib: a second build of the library (python -m secp256k1_zkp_amd.build_lib -o OTHER.so -DS2K_PK_FOLD_FUSED=0: the load-then-fold
chain) is loaded next to the product library and the combine calls alternate between the two, five pairs per shape; the fused first
pass is a gain where the two ranges are disjoint (the rule of DESIGN.md 4.2).

Inputs.  The keys are n distinct points x_i G made by the engine's own s2k_ecmult_batch; every item and set is served, and the first
results are compared with integer arithmetic in Python."""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from secp256k1_zkp_amd.constants import G_XY  # noqa: E402

P_FIELD = 2 ** 256 - 2 ** 32 - 977


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def compact(obj):
    """JSON with one line per innermost object or list"""
    flat = lambda m: re.sub(r"\s*\n\s*", " ", m.group(0))      # noqa: E731
    return re.sub(r"\{[^{}\[\]]*\}|\[[^{}\[\]]*\]", flat, json.dumps(obj, indent=1))


def _add(a, b):
    """affine addition over integers (distinct, finite points)"""
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P_FIELD) % P_FIELD
    x = (lam * lam - a[0] - b[0]) % P_FIELD
    return x, (lam * (a[0] - x) - a[1]) % P_FIELD


def _pt(xy):
    return int.from_bytes(xy[:32].tobytes(), "big"), int.from_bytes(xy[32:].tobytes(), "big")


def _obj(p):
    return p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


class OtherLib:
    """a second build of the library, loaded beside the product one: its own engine, the combine `_dev` call alone"""

    def __init__(self, path):
        self.lib = L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.s2k_engine_create.restype = vp; L.s2k_engine_create.argtypes = [ctypes.c_int]
        L.s2k_engine_destroy.argtypes = [vp]
        L.s2k_engine_sync.argtypes = [vp]
        L.s2k_engine_last_ms.restype = ctypes.c_float; L.s2k_engine_last_ms.argtypes = [vp, ctypes.c_int]
        L.secp256k1_ec_pubkey_combine_batch_dev.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, sz]
        self.h = L.s2k_engine_create(0)
        assert self.h, "the second library's engine"

    def combine(self, res, out, keys, off, key_format):
        ok = self.lib.secp256k1_ec_pubkey_combine_batch_dev(self.h, None, res.data_ptr(), out.data_ptr(), 1, None, keys.data_ptr(), key_format,
                                                            off.ctypes.data_as(ctypes.c_void_p), off.size - 1)
        assert ok == 1, "the second library's combine call failed"

    def sync_ms(self):
        assert self.lib.s2k_engine_sync(self.h) == 1
        return float(self.lib.s2k_engine_last_ms(self.h, 0))

    def close(self):
        self.lib.s2k_engine_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--set-sizes", type=int, nargs="+", default=[2, 16, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ab-lib", default=None, help="a second build of the library (-DS2K_PK_FOLD_FUSED=0) for the A/B of the fused first pass")
    ap.add_argument("--reference-us", default=None, help="the reference's per-item times on one core, measured through tests/pubkey_ref.py where its build is: recorded as given")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(45)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    other = OtherLib(a.ab_lib) if a.ab_lib else None
    nmax = max(a.sizes)

    def scalars(k):
        s = rng.integers(0, 256, (k, 32), dtype=np.uint8); s[:, 0] &= 0x7F; s[:, 31] |= 1      # in [1, 2^255): below n, nonzero
        return s
    X = eng.ecmult_batch(np.tile(np.frombuffer(G_XY, np.uint8), (nmax, 1)), np.zeros((nmax, 32), np.uint8), ng=scalars(nmax))[0]      # n x (x | y), big-endian
    ser = np.concatenate([(2 + (X[:, 63] & 1))[:, None], X[:, :32]], axis=1).astype(np.uint8)
    gser = ser.copy(); gser[:, 0] = 0x0a                                                     # the same x as a serialised generator
    obj = np.ascontiguousarray(np.concatenate([X[:, 31::-1], X[:, :31:-1]], axis=1))
    magic = np.frombuffer(bytes([0xf5, 0x7a, 0x3d, 0xa0]), np.uint8)
    nonces = np.concatenate([np.tile(magic, (nmax, 1)), obj, np.roll(obj, 1, axis=0)], axis=1)
    tw = scalars(nmax)
    d_xy, d_ser, d_gser, d_obj, d_non, d_tw = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (X, ser, gser, obj, nonces, tw))
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "timing": "s2k_engine_last_ms(0), the whole launch chain of a call", "sizes": {}}
    if other:
        out["ab_library"] = {"file": os.path.basename(a.ab_lib), "so_sha256": hashlib.sha256(open(a.ab_lib, "rb").read()).hexdigest(), "flag": "-DS2K_PK_FOLD_FUSED=0", "pairs": 5}
    for n in a.sizes:
        row = {}
        res = torch.zeros(n, dtype=torch.int32, device=dev); o64 = torch.zeros((n, 64), dtype=torch.uint8, device=dev); o33 = torch.zeros((n, 33), dtype=torch.uint8, device=dev)
        g64 = torch.zeros((n, 64), dtype=torch.uint8, device=dev); g33 = torch.zeros((n, 33), dtype=torch.uint8, device=dev); gres = torch.zeros(n, dtype=torch.int32, device=dev)
        r_xy = torch.zeros((n, 64), dtype=torch.uint8, device=dev); r_inf = torch.zeros(n, dtype=torch.int32, device=dev)
        t64 = torch.zeros((n, 64), dtype=torch.uint8, device=dev); tres = torch.zeros(n, dtype=torch.int32, device=dev)
        calls = {
            "convert_2_to_1": (lambda: eng.pubkey_convert_dev(res, o64, d_ser[:n], 2, 1), n),
            "generator_parse": (lambda: eng.generator_parse_batch_dev(gres, g64, d_gser[:n]), n),
            "convert_1_to_2": (lambda: eng.pubkey_convert_dev(res, o33, d_obj[:n], 1, 2), n),
            "generator_serialize": (lambda: eng.generator_serialize_batch_dev(g33, g64), n),
            "tweak_mul_1_to_1": (lambda: eng.pubkey_tweak_mul_dev(tres, t64, d_obj[:n], d_tw[:n]), n),
            "ecmult_batch": (lambda: eng.ecmult_batch_dev(r_xy, r_inf, d_xy[:n], d_tw[:n]), n),
        }
        ab = {}
        for m in a.set_sizes:
            if m > n:
                continue
            ns = n // m
            off = np.arange(0, ns * m + 1, m, dtype=np.uint64)
            cres = torch.zeros(ns, dtype=torch.int32, device=dev); cout = torch.zeros((ns, 64), dtype=torch.uint8, device=dev)
            nres = torch.zeros(ns, dtype=torch.int32, device=dev); nout = torch.zeros((ns, 132), dtype=torch.uint8, device=dev)
            for f, keys in ((1, d_obj), (2, d_ser)):
                name = "combine_%dkey_format%d" % (m, f)
                calls[name] = ((lambda keys=keys, f=f, cres=cres, cout=cout, off=off, k=ns * m: eng.pubkey_combine_dev(cres, cout, keys[:k], off, key_format=f, out_format=1)), ns * m)
                if other:
                    ab[name] = (calls[name][0], (lambda keys=keys, f=f, cres=cres, cout=cout, off=off, k=ns * m: other.combine(cres, cout, keys[:k], off, f)), ns * m)
            calls["nonce_agg_%d_per_session" % m] = ((lambda nres=nres, nout=nout, off=off, k=ns * m: eng.musig_nonce_agg_dev(nres, nout, d_non[:k], off, nonce_format=1, out_format=1)), ns * m)
            if m == 2:
                chk = (cres, cout)
        for w in range(2):
            for name, (call, items) in calls.items():
                call(); eng.sync()
            assert bool(res.all()) and bool(gres.all()) and bool(tres.all()) and bool(chk[0].all()), "an item was refused"
            assert bytes(o33[0].cpu().numpy()) == ser[0].tobytes() and bytes(o64[0].cpu().numpy()) == obj[0].tobytes(), "convert: wrong bytes"
            assert bytes(chk[1][0].cpu().numpy()) == _obj(_add(_pt(X[0]), _pt(X[1]))), "combine: wrong sum"
            assert bytes(t64[0].cpu().numpy()) == bytes(np.concatenate([r_xy[0, :32].cpu().numpy()[::-1], r_xy[0, 32:].cpu().numpy()[::-1]])), "tweak_mul differs from ecmult_batch"
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, (call, items) in calls.items():
                call(); eng.sync(); ms[name].append(eng.last_ms(0))
        for name, (call, items) in calls.items():
            row[name] = stats(ms[name], items)
            if name.startswith("nonce_agg"):
                row[name]["ms_median_per_column"] = round(row[name]["ms_median"] / 2, 4)
        per = lambda k: row[k]["ms_median"] / calls[k][1]      # noqa: E731
        row["ratios"] = {"convert_2_to_1_over_generator_parse": round(per("convert_2_to_1") / per("generator_parse"), 3),
                         "convert_1_to_2_over_generator_serialize": round(per("convert_1_to_2") / per("generator_serialize"), 3),
                         "tweak_mul_over_ecmult_batch": round(per("tweak_mul_1_to_1") / per("ecmult_batch"), 3)}
        for m in a.set_sizes:
            for f in (1, 2):
                k = "combine_%dkey_format%d" % (m, f)
                if k in row:
                    row["ratios"][k + "_over_nonce_agg_column"] = round(row[k]["ms_median"] / row["nonce_agg_%d_per_session" % m]["ms_median_per_column"], 3)
        if ab:
            row["fused_first_pass_ab"] = {}
            for name, (fa, fb, items) in ab.items():
                fb(); other.sync_ms()
                ta, tb = [], []
                for _ in range(5):
                    fa(); eng.sync(); ta.append(eng.last_ms(0))
                    fb(); tb.append(other.sync_ms())
                disjoint = max(ta) < min(tb) or max(tb) < min(ta)
                row["fused_first_pass_ab"][name] = {"fused_ms": [round(v, 4) for v in sorted(ta)], "load_then_fold_ms": [round(v, 4) for v in sorted(tb)],
                                                    "verdict": ("fused faster" if max(ta) < min(tb) else "load-then-fold faster") if disjoint else "ranges overlap: not resolved"}
        out["sizes"][str(n)] = row
    eng.close()
    if other:
        other.close()
    out["reference_cpu_us_per_item"] = a.reference_us or "not measured here: see README (measured through tests/pubkey_ref.py where the reference's build is)"
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
