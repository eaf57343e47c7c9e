#!/usr/bin/env python3
"""Device-resident timing of k_adaptor_verify through secp256k1_ecdsa_adaptor_verify_batch_dev, next to k_ecdsa_verify
(secp256k1_ecdsa_verify_batch_dev) in the same process, on the same box, at the same n:

    python tools/adaptor_bare.py [--sizes 65536 1048576] [--rounds 3] [--out profiles/adaptor_rates.json]
    python tools/adaptor_bare.py --ab two_call.so [--ab-rounds 3] ...     (two_call.so: python -m secp256k1_zkp_amd.build_lib -o two_call.so -DS2K_ADAPTOR_JOINT=0)

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)).  After two warm-up calls of each, the two
kernels alternate for --rounds rounds; every figure is the median of the rounds with their minimum and maximum (the spread) beside it.
--ab runs the largest size again in child processes that alternate between the default library (joint form) and the given one (two-call
form), in the way of tools/ab_probe.py, and records both rates and their spreads.

Inputs.  Every item is a distinct valid adaptor signature: the points (X = x G, Y = y G, R' = k G, R = k Y and the two commitments of
the DLEQ proof) come from the engine's own s2k_ecmult_batch, the challenges from hashlib and the scalars from Python integers with one
shared modular inversion.  One item in 256 has a bit of its message flipped: it runs every stage and fails the last comparison.  The ECDSA
items are made from the same keys and nonces (r = x(R') mod n, low s).  All verdicts are checked."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def batch_inverse(vals):
    """1/v mod n for every v (none zero) with one modular inversion"""
    pre, run = [], 1
    for v in vals:
        pre.append(run); run = run * v % N
    inv = pow(run, -1, N)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % N; inv = inv * vals[i] % N
    return out


def make_items(eng, n, rng):
    """-> dict of uint8 arrays: adaptor sigs (n,162), pk (n,33), msg (n,32), ek (n,33), ECDSA compact sigs (n,64); expected adaptor verdicts"""
    def scalars():
        a = rng.integers(0, 256, (n, 32), dtype=np.uint8); a[:, 0] &= 0x7F; a[:, 31] |= 1      # in [1, 2^255): below n, nonzero
        return a
    ints = lambda a: [int.from_bytes(r.tobytes(), "big") for r in a]      # noqa: E731
    x, y, k, kd = scalars(), scalars(), scalars(), scalars()
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    g = np.tile(np.frombuffer(G_XY, np.uint8), (n, 1)); zero = np.zeros((n, 32), np.uint8)
    gmul = lambda s: eng.ecmult_batch(g, zero, ng=s)[0]                   # noqa: E731
    X, Y, Rp, T1 = gmul(x), gmul(y), gmul(k), gmul(kd)
    R, T2 = eng.ecmult_batch(Y, k)[0], eng.ecmult_batch(Y, kd)[0]
    ser = lambda P: np.concatenate([(2 + (P[:, 63] & 1))[:, None], P[:, :32]], axis=1).astype(np.uint8)      # noqa: E731
    sX, sY, sRp, sR, sT1, sT2 = (ser(P) for P in (X, Y, Rp, R, T1, T2))
    tag = hashlib.sha256(b"DLEQ").digest() * 2
    xi, ki, kdi, mi = ints(x), ints(k), ints(kd), ints(msg)
    kinv = batch_inverse(ki)
    sigs = np.zeros((n, 162), np.uint8); esig = np.zeros((n, 64), np.uint8)
    for i in range(n):
        e = int.from_bytes(hashlib.sha256(tag + sRp[i].tobytes() + sY[i].tobytes() + sR[i].tobytes() + sT1[i].tobytes() + sT2[i].tobytes()).digest(), "big") % N
        s = (kdi[i] + e * ki[i]) % N
        m = mi[i] % N
        sp = (m + (int.from_bytes(sR[i, 1:].tobytes(), "big") % N) * xi[i]) * kinv[i] % N
        r2 = int.from_bytes(sRp[i, 1:].tobytes(), "big") % N
        s2 = (m + r2 * xi[i]) * kinv[i] % N
        s2 = min(s2, N - s2)
        assert sp and r2 and s2
        sigs[i] = np.frombuffer(sR[i].tobytes() + sRp[i].tobytes() + sp.to_bytes(32, "big") + e.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint8)
        esig[i] = np.frombuffer(r2.to_bytes(32, "big") + s2.to_bytes(32, "big"), np.uint8)
    amsg = msg.copy(); exp = np.ones(n, np.int32)
    bad = np.arange(255, n, 256)
    amsg[bad, 31] ^= 1; exp[bad] = 0
    return dict(sig=sigs, pk=sX, msg=amsg, ek=sY, esig=esig, emsg=msg), exp


def measure(eng, D, exp, n, rounds):
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev)      # noqa: E731
    d = {k: T(v) for k, v in D.items()}
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    ad = lambda: eng.ecdsa_adaptor_verify_batch_dev(res, d["sig"], d["pk"], d["msg"], d["ek"], pk_format=0, n=n)      # noqa: E731
    ec = lambda: eng.ecdsa_verify_batch_dev(res, d["esig"], d["emsg"], d["pk"], n=n)                                  # noqa: E731
    for _ in range(2):
        ad(); eng.sync()
        assert np.array_equal(res.cpu().numpy(), exp[:n]), "k_adaptor_verify: wrong verdicts"
        ec(); eng.sync()
        assert res.cpu().numpy().all(), "k_ecdsa_verify: wrong verdicts"
    a_ms, e_ms = [], []
    for _ in range(rounds):
        ad(); eng.sync(); a_ms.append(eng.last_ms(1))
        ec(); eng.sync(); e_ms.append(eng.last_ms(1))
    row = {"adaptor_verify": stats(a_ms, n), "ecdsa_verify": stats(e_ms, n)}
    row["adaptor_item_time_over_ecdsa_item_time"] = round(row["adaptor_verify"]["ms_median"] / row["ecdsa_verify"]["ms_median"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", default=None, help="a library built with -DS2K_ADAPTOR_JOINT=0 to alternate with")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-size", type=int, default=1 << 18, help="items per call in the A/B children (each child makes its own inputs)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    rng = np.random.default_rng(41)
    eng = Engine(0)
    D, exp = make_items(eng, max(a.sizes), rng)
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "corrupted_one_in": 256, "sizes": {}}
    for n in a.sizes:
        out["sizes"][str(n)] = measure(eng, D, exp, n, a.rounds)
    eng.close()
    if a.child:
        print("RESULT " + json.dumps(out["sizes"][str(max(a.sizes))]["adaptor_verify"]))
        return
    if a.ab:
        n = a.ab_size
        libs = {"joint (default library)": _native.LIB_PATH, "two-call (-DS2K_ADAPTOR_JOINT=0)": os.path.abspath(a.ab)}
        runs = {k: [] for k in libs}
        for _ in range(a.ab_rounds):
            for name, lib in libs.items():
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", str(n), "--rounds", str(a.rounds)], env=dict(os.environ, S2K_LIB=lib),
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if not line:
                    raise SystemExit("child failed (%s): %s" % (name, p.stderr[-800:]))
                runs[name].append(json.loads(line[0][7:]))
        ab = {"n": n, "runs": runs}
        med = {k: sorted(r["ms_median"] for r in v)[len(v) // 2] for k, v in runs.items()}
        spread = {k: round(100 * (max(r["ms_max"] for r in v) - min(r["ms_min"] for r in v)) / med[k], 2) for k, v in runs.items()}
        j, t = med["joint (default library)"], med["two-call (-DS2K_ADAPTOR_JOINT=0)"]
        ab["ms_median"] = med; ab["spread_pct"] = spread
        ab["joint_faster_by_pct"] = round(100 * (t - j) / t, 2)
        ab["joint_stays_default"] = bool(100 * (t - j) / t > max(spread.values()))
        out["joint_vs_two_call"] = ab
    out["reference_cpu_adaptor_verify"] = ("not measured here: the reference's module is only compiled by tests/golden/make_adaptor_golden.py --time, "
                                           "which needs the reference's sources")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
