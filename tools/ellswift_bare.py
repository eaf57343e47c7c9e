#!/usr/bin/env python3
"""Device-resident timing of the ElligatorSwift kernels next to the kernels they are closest to, in the same process, on the same box, at
the same n:

    python tools/ellswift_bare.py [--sizes 65536 1048576] [--rounds 5] [--model-items 4096] [--out profiles/ellswift_rates.json]

    k_ellswift_decode  (secp256k1_ellswift_decode_batch_dev) in its three output formats: x only (two roots and the wave-shared
                       inversion), key objects and compressed keys (three roots and the inversion)
    k_ellswift_encode  (secp256k1_ellswift_encode_batch_dev) with object and with compressed keys: the plain form of the loop, one item
                       per lane, a wavefront running as many rounds as the slowest of its 64 items needs
    next to            k_gen_parse (secp256k1_generator_parse_batch_dev: one root per item), k_gen_generate
                       (secp256k1_generator_generate_batch_dev: the other map the engine has, six roots and two inversions) and
                       k_ecdsa_verify (secp256k1_ecdsa_verify_batch_dev)

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)).  After two warm-up calls of each, the calls
alternate for --rounds rounds; every figure is the median of the rounds with their minimum and maximum (the spread) beside it.

Inputs.  Decode: seeded random 64-byte strings.  Encode: 64 public keys (Python integers) cycled over the items with seeded random
rnd32, so every item has its own hash stream.  ECDSA: distinct valid signatures (points from the engine's own s2k_ecmult_batch).  Every
output is checked: the decode formats against each other and the Python model on a sample, encode by decoding back on the device to the
key that went in, the sample byte for byte against the model.  The model (tests/ellswift_ref.py) also gives, for the first
--model-items encode items, the mean number of attempts per item and the mean number of rounds per wavefront: what the loop's waiting
costs."""
import argparse
import hashlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402
from tests import ellswift_ref as E  # noqa: E402


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def ratio(row, a, b):
    """per-item time of a over b with the range the rounds allow"""
    return {"median": round(row[a]["ms_median"] / row[b]["ms_median"], 3), "min": round(row[a]["ms_min"] / row[b]["ms_max"], 3),
            "max": round(row[a]["ms_max"] / row[b]["ms_min"], 3)}


def batch_inverse(vals):
    pre, run = [], 1
    for v in vals:
        pre.append(run); run = run * v % N
    inv = pow(run, -1, N)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % N; inv = inv * vals[i] % N
    return out


def make_items(eng, n, rng):
    prng = random.Random(324)
    pts = [E.pt_mul(prng.randrange(1, N), E.G) for _ in range(64)]
    k33 = np.frombuffer(b"".join(E.ser33(*p) for p in pts), np.uint8).reshape(64, 33)
    k64 = np.frombuffer(b"".join(E.pubkey_object(*p) for p in pts), np.uint8).reshape(64, 64)
    idx = np.arange(n) % 64
    D = dict(ell=rng.integers(0, 256, (n, 64), dtype=np.uint8), key33=k33[idx], key64=k64[idx], rnd=rng.integers(0, 256, (n, 32), dtype=np.uint8),
             gen33=np.concatenate([np.full((n, 1), 0x0a, np.uint8), k33[idx][:, 1:]], axis=1), asset=rng.integers(0, 256, (n, 32), dtype=np.uint8))

    def scalars():
        a = rng.integers(0, 256, (n, 32), dtype=np.uint8); a[:, 0] &= 0x3F; a[:, 31] |= 1
        return a
    ints = lambda a: [int.from_bytes(r.tobytes(), "big") for r in a]      # noqa: E731
    d, k = scalars(), scalars()
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    g = np.tile(np.frombuffer(G_XY, np.uint8), (n, 1)); zero = np.zeros((n, 32), np.uint8)
    gmul = lambda s: eng.ecmult_batch(g, zero, ng=s)[0]                   # noqa: E731
    X, R = gmul(d), gmul(k)
    di, ki, mi = ints(d), ints(k), ints(msg)
    kinv = batch_inverse(ki)
    sig = np.zeros((n, 64), np.uint8)
    for i in range(n):
        r = int.from_bytes(R[i, :32].tobytes(), "big") % N
        s = (mi[i] % N + r * di[i]) * kinv[i] % N
        s = min(s, N - s)
        sig[i] = np.frombuffer(r.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint8)
    D.update(sig=sig, msg=msg, pk=np.concatenate([(2 + (X[:, 63] & 1))[:, None], X[:, :32]], axis=1).astype(np.uint8))
    return D


def model_figures(D, m):
    """the model on the first m encode items: attempts per item, rounds per wavefront of 64, and the bytes the engine must produce"""
    att, ells = [], []
    for i in range(m):
        r, ell, a, _ = E.encode(D["key33"][i].tobytes(), 2, D["rnd"][i].tobytes())
        assert r == 1
        att.append(a); ells.append(ell)
    return att, ells


def measure(eng, D, n, rounds, sample):
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(v[:n])).to(dev) for k, v in D.items()}
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    o32 = torch.zeros((n, 32), dtype=torch.uint8, device=dev); o33 = torch.zeros((n, 33), dtype=torch.uint8, device=dev)
    o64 = torch.zeros((n, 64), dtype=torch.uint8, device=dev); ell = torch.zeros((n, 64), dtype=torch.uint8, device=dev); back = torch.zeros((n, 33), dtype=torch.uint8, device=dev)
    calls = {
        "decode_x_only": lambda: eng.ellswift_decode_dev(o32, d["ell"], out_format=0, n=n),
        "decode_object": lambda: eng.ellswift_decode_dev(o64, d["ell"], out_format=1, n=n),
        "decode_compressed": lambda: eng.ellswift_decode_dev(o33, d["ell"], out_format=2, n=n),
        "encode_object_keys": lambda: eng.ellswift_encode_dev(res, ell, d["key64"], d["rnd"], key_format=1, n=n),
        "encode_compressed_keys": lambda: eng.ellswift_encode_dev(res, ell, d["key33"], d["rnd"], key_format=2, n=n),
        "generator_parse": lambda: eng.generator_parse_batch_dev(res, o64, d["gen33"], n=n),
        "generator_generate": lambda: eng.generator_generate_batch_dev(res, o64, d["asset"], n=n),
        "ecdsa_verify": lambda: eng.ecdsa_verify_batch_dev(res, d["sig"], d["msg"], d["pk"], n=n),
    }
    for _ in range(2):
        for name, call in calls.items():
            call(); eng.sync()
            if name.startswith("encode"):
                assert bool(res.all()), name + ": an item was refused"
                eng.ellswift_decode_dev(back, ell, out_format=2, n=n); eng.sync()
                assert torch.equal(back, d["key33"]), name + ": an encoding does not decode to its key"
                m = min(n, len(sample))
                assert ell[:m].cpu().numpy().tobytes() == b"".join(sample[:m]), name + ": differs from the model"
            elif name in ("generator_parse", "ecdsa_verify", "generator_generate"):
                assert bool(res.all()), name + ": wrong verdicts"
    x, obj, comp = o32.cpu().numpy(), None, o33.cpu().numpy()
    eng.ellswift_decode_dev(o64, d["ell"], out_format=1, n=n); eng.sync(); obj = o64.cpu().numpy()
    assert np.array_equal(obj[:, 31::-1], x) and np.array_equal(comp[:, 1:], x) and np.array_equal(comp[:, 0], 2 + (obj[:, 32] & 1)), "decode formats disagree"
    for i in range(min(n, 64)):
        assert obj[i].tobytes() == E.decode_out(D["ell"][i].tobytes(), 1), "decode differs from the model"
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            call(); eng.sync(); ms[name].append(eng.last_ms(1))
    row = {k: stats(v, n) for k, v in ms.items()}
    row["item_time_ratios"] = {
        "decode_x_only_over_generator_parse": ratio(row, "decode_x_only", "generator_parse"),
        "decode_object_over_generator_parse": ratio(row, "decode_object", "generator_parse"),
        "decode_object_over_decode_x_only": ratio(row, "decode_object", "decode_x_only"),
        "decode_object_over_generator_generate": ratio(row, "decode_object", "generator_generate"),
        "decode_object_over_ecdsa_verify": ratio(row, "decode_object", "ecdsa_verify"),
        "encode_compressed_over_generator_parse": ratio(row, "encode_compressed_keys", "generator_parse"),
        "encode_compressed_over_generator_generate": ratio(row, "encode_compressed_keys", "generator_generate"),
        "encode_compressed_over_ecdsa_verify": ratio(row, "encode_compressed_keys", "ecdsa_verify"),
        "encode_compressed_over_decode_object": ratio(row, "encode_compressed_keys", "decode_object"),
        "encode_object_over_encode_compressed": ratio(row, "encode_object_keys", "encode_compressed_keys"),
    }
    row["root_worth_ms"] = round(row["generator_parse"]["ms_median"], 4)
    row["decode_object_minus_x_only_ms"] = round(row["decode_object"]["ms_median"] - row["decode_x_only"]["ms_median"], 4)
    return row


def reference_cpu(us):
    if us is None:
        return "not measured here: the reference's module is only compiled by tests/golden/make_ellswift_golden.py --time, which needs the reference's sources"
    return {"secp256k1_ellswift_decode_us_per_call": us[0], "secp256k1_ellswift_encode_us_per_call": us[1],
            "note": "tests/golden/make_ellswift_golden.py --time on one core of the build box, ctypes call overhead included; handed in with --reference-us"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model-items", type=int, default=4096)
    ap.add_argument("--reference-us", type=float, nargs=2, default=None, metavar=("DECODE", "ENCODE"),
                    help="what tests/golden/make_ellswift_golden.py --time printed on the build box, recorded beside the rates")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    rng = np.random.default_rng(324)
    eng = Engine(0)
    D = make_items(eng, max(a.sizes), rng)
    m = min(a.model_items, max(a.sizes))
    att, sample = model_figures(D, m)
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "model": {"items": m, "mean_attempts_per_item": round(sum(att) / m, 3), "max_attempts": max(att),
                     "mean_rounds_per_wavefront": round(E.rounds_per_wavefront(att), 3),
                     "note": "tests/ellswift_ref.py on the first `items` encode inputs: a wavefront of the one-item-per-lane loop runs as many rounds as the slowest of its 64 items"},
           "loop_forms": "one (the plain form: one item per lane); no second form was built, so there is no choice to record",
           "sizes": {}}
    for n in a.sizes:
        out["sizes"][str(n)] = measure(eng, D, n, a.rounds, sample)
    out["ellswift_capped"] = eng.ellswift_capped()
    eng.close()
    out["reference_cpu"] = reference_cpu(a.reference_us)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
