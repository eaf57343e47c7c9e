#!/usr/bin/env python3
"""Device-resident timing of the sign-to-contract kernels, each next to the kernel it is closest to, in the same process, on the same box,
at the same n:

    python tools/s2c_bare.py [--sizes 65536 1048576] [--rounds 5] [--out profiles/s2c_rates.json]

    k_s2c_commit       (secp256k1_ecdsa_s2c_verify_commit_batch_dev)   next to  k_tweak_add (secp256k1_pubkey_tweak_add_batch_dev, compressed
                       keys): the same lift, the same table walk and the same addition, with an inversion where this has a hash
    host verification  (secp256k1_anti_exfil_host_verify_batch_dev) in both forms, the fused k_s2c_host_verify (S2K_OPT_S2C_FUSED) and the chain
                       k_s2c_commit -> k_s2c_ecdsa_and,        next to  k_ecdsa_verify (secp256k1_ecdsa_verify_batch_dev)
    and the fused form against the SUM of k_s2c_commit and k_ecdsa_verify on the same items: what a two-kernel chain costs.  The rule: the
    fused form is the default only if it is faster than that sum by more than the larger of the two spreads.

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)).  After two warm-up calls of each, the five
calls alternate for --rounds rounds; every figure is the median of the rounds with their minimum and maximum (the spread) beside it.

Inputs.  Every item is a distinct valid sign-to-contract signature: the points (X = d G, the opening O = k G, R = (k + t) G) come from the
engine's own s2k_ecmult_batch, the tweaks t from hashlib and the scalars from Python integers with one shared modular inversion.  One
item in 256 has a bit of its data flipped: it runs every stage and fails the comparison.  All verdicts are checked, and the tweak-add
call's outputs are checked to be R."""
import argparse
import hashlib
import json
import os
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
    """-> dict of uint8 arrays: compact sigs (n,64), msg (n,32), pk (n,33), data (n,32) with one in 256 corrupted, openings (n,33), tweaks (n,32),
    R as (n,64) x | y big-endian; and the expected verdicts"""
    def scalars():
        a = rng.integers(0, 256, (n, 32), dtype=np.uint8); a[:, 0] &= 0x3F; a[:, 31] |= 1      # in [1, 2^254): k + t stays nonzero mod n
        return a
    ints = lambda a: [int.from_bytes(r.tobytes(), "big") for r in a]      # noqa: E731
    d, k = scalars(), scalars()
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8); data = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    g = np.tile(np.frombuffer(G_XY, np.uint8), (n, 1)); zero = np.zeros((n, 32), np.uint8)
    gmul = lambda s: eng.ecmult_batch(g, zero, ng=s)[0]                   # noqa: E731
    ser = lambda P: np.concatenate([(2 + (P[:, 63] & 1))[:, None], P[:, :32]], axis=1).astype(np.uint8)      # noqa: E731
    X, O = gmul(d), gmul(k)
    sX, sO = ser(X), ser(O)
    tag = hashlib.sha256(b"s2c/ecdsa/point").digest() * 2
    di, ki, mi = ints(d), ints(k), ints(msg)
    tw = np.zeros((n, 32), np.uint8); kk = []
    for i in range(n):
        t = hashlib.sha256(tag + sO[i].tobytes() + data[i].tobytes()).digest()
        ti = int.from_bytes(t, "big")
        assert ti < N and (ki[i] + ti) % N
        tw[i] = np.frombuffer(t, np.uint8); kk.append((ki[i] + ti) % N)
    R = gmul(np.frombuffer(b"".join(v.to_bytes(32, "big") for v in kk), np.uint8).reshape(n, 32))
    kinv = batch_inverse(kk)
    sig = np.zeros((n, 64), np.uint8)
    for i in range(n):
        r = int.from_bytes(R[i, :32].tobytes(), "big") % N
        s = (mi[i] % N + r * di[i]) * kinv[i] % N
        s = min(s, N - s)
        assert r and s
        sig[i] = np.frombuffer(r.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint8)
    bdata = data.copy(); exp = np.ones(n, np.int32)
    bad = np.arange(255, n, 256)
    bdata[bad, 31] ^= 1; exp[bad] = 0
    return dict(sig=sig, msg=msg, pk=sX, data=bdata, op=sO, tw=tw, R=R), exp


def measure(eng, D, exp, n, rounds):
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev)      # noqa: E731
    d = {k: T(v) for k, v in D.items()}
    res = torch.zeros(n, dtype=torch.int32, device=dev); pko = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    def host_verify(fused):
        eng.set_option(Engine.OPT_S2C_FUSED, fused)
        try:
            eng.anti_exfil_host_verify_batch_dev(res, d["sig"], d["msg"], d["pk"], d["data"], d["op"], n=n)
        finally:
            eng.set_option(Engine.OPT_S2C_FUSED, 0)
    calls = {
        "s2c_commit": lambda: eng.ecdsa_s2c_verify_commit_batch_dev(res, d["sig"], d["data"], d["op"], n=n),
        "tweak_add_compressed": lambda: eng.pubkey_tweak_add_batch_dev(res, pko, d["op"], d["tw"], key_format=2, n=n),
        "s2c_host_verify_fused": lambda: host_verify(1),
        "s2c_host_verify_chain": lambda: host_verify(0),
        "ecdsa_verify": lambda: eng.ecdsa_verify_batch_dev(res, d["sig"], d["msg"], d["pk"], n=n),
    }
    want = {"s2c_commit": exp[:n], "s2c_host_verify_fused": exp[:n], "s2c_host_verify_chain": exp[:n], "tweak_add_compressed": np.ones(n, np.int32),
            "ecdsa_verify": np.ones(n, np.int32)}
    for _ in range(2):
        for name, call in calls.items():
            call(); eng.sync()
            assert np.array_equal(res.cpu().numpy(), want[name]), name + ": wrong verdicts"
            if name == "tweak_add_compressed":                                       # the objects are x | y little-endian: R
                assert np.array_equal(pko.cpu().numpy().reshape(n, 2, 32)[:, :, ::-1].reshape(n, 64), D["R"][:n]), "tweak_add: wrong points"
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            call(); eng.sync(); ms[name].append(eng.last_ms(1))
    row = {k: stats(v, n) for k, v in ms.items()}
    row["commit_item_time_over_tweak_add_item_time"] = round(row["s2c_commit"]["ms_median"] / row["tweak_add_compressed"]["ms_median"], 3)
    row["fused_host_verify_item_time_over_ecdsa_item_time"] = round(row["s2c_host_verify_fused"]["ms_median"] / row["ecdsa_verify"]["ms_median"], 3)
    row["chain_host_verify_item_time_over_ecdsa_item_time"] = round(row["s2c_host_verify_chain"]["ms_median"] / row["ecdsa_verify"]["ms_median"], 3)
    both = [a + b for a, b in zip(ms["s2c_commit"], ms["ecdsa_verify"])]                 # round by round: the two kernels a chain is made of, each on its own
    cs = stats(both, n)
    fused = row["s2c_host_verify_fused"]
    faster = 100 * (cs["ms_median"] - fused["ms_median"]) / cs["ms_median"]
    spread = max(cs["spread_pct"], fused["spread_pct"])
    row["fused_vs_sum"] = {"commit_plus_ecdsa": cs, "fused_faster_by_pct": round(faster, 2), "larger_spread_pct": spread, "fused_is_default": bool(faster > spread)}
    row["fused_faster_than_the_chain_as_launched_by_pct"] = round(100 * (row["s2c_host_verify_chain"]["ms_median"] - fused["ms_median"]) / row["s2c_host_verify_chain"]["ms_median"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    rng = np.random.default_rng(43)
    eng = Engine(0)
    D, exp = make_items(eng, max(a.sizes), rng)
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "corrupted_one_in": 256, "sizes": {}}
    for n in a.sizes:
        out["sizes"][str(n)] = measure(eng, D, exp, n, a.rounds)
    eng.close()
    out["fused_is_default"] = all(v["fused_vs_sum"]["fused_is_default"] for v in out["sizes"].values())      # the rule; the library's default follows it
    out["reference_cpu"] = ("not measured here: the reference's module is only compiled by tests/golden/make_s2c_golden.py --time, which needs the reference's sources")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
