#!/usr/bin/env python3
"""Device-resident timing of the batch half-aggregate calls next to their yardsticks, in one process over the same signatures:

    python tools/halfagg_batch_bare.py [--sigs 65536] [--agg-sizes 2 16 256] [--rounds 5] [--loop-max 256] [--out profiles/halfagg_batch_rates.json]

Per aggregate size m (the --sigs signatures cut into aggregates of m):
  aggregate_batch   secp256k1_schnorrsig_aggregate_batch_dev; its chain kernel alone is s2k_engine_last_ms(1)
  aggverify_batch   secp256k1_schnorrsig_aggverify_batch_dev on the aggregates the call above made (every verdict must be 1)
  single_loop       the first --loop-max of the same aggregates as a loop of secp256k1_schnorrsig_aggverify_dev calls, and the batch call
                    on exactly those aggregates next to it
  verify_unaggregated   secp256k1_schnorrsig_verify_batch_dev on the same signatures, not aggregated
Times are wall-clock milliseconds from before the call to after s2k_engine_sync (a loop of calls has no single pair of events; the
batch verifier waits once for its offsets on the host, which wall-clock time includes), after two warm-up calls of each; the calls
alternate for --rounds rounds and every figure is the median with the minimum and maximum beside it.  The chain kernel's share of the
batch verifier is the chain kernel's event time in the aggregation call -- the same kernel over the same bytes -- over the verifier's
median.

THE CONDITION (asserted, exit status 1): at 256 aggregates of 16 signatures the batch verifier is faster than the loop of single calls,
the two ranges clear of each other (the slowest batch round below the fastest loop round).

Signatures are made here (BIP-340 with public test keys: the engine's s2k_ecmult_batch gives x_i G and k_i G, Python the challenges
and s_i); every signature is checked by the unaggregated verifier before anything is timed."""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from secp256k1_zkp_amd.api import _dp, _p  # noqa: E402
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402


def stats(ms, items):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "signatures_per_s": round(items / med * 1e3, 1)}


def compact(obj):
    flat = lambda m: re.sub(r"\s*\n\s*", " ", m.group(0))      # noqa: E731
    return re.sub(r"\{[^{}\[\]]*\}|\[[^{}\[\]]*\]", flat, json.dumps(obj, indent=1))


def ctypes_ptr(t, byte_off):
    return ctypes.c_void_p(t.data_ptr() + byte_off)


def make_signatures(eng, rng, n):
    """n BIP-340 signatures over random messages: (sigs (n,64), msgs (n,32), keys (n,32))"""
    def scalars():
        s = rng.integers(0, 256, (n, 32), dtype=np.uint8); s[:, 0] &= 0x7F; s[:, 31] |= 1
        return s
    g = np.tile(np.frombuffer(G_XY, np.uint8), (n, 1)); zero = np.zeros((n, 32), np.uint8)
    sk, k = scalars(), scalars()
    Pk = eng.ecmult_batch(g, zero, ng=sk)[0]; R = eng.ecmult_batch(g, zero, ng=k)[0]
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    tag = hashlib.sha256(b"BIP0340/challenge").digest() * 2
    sigs = np.zeros((n, 64), np.uint8)
    for i in range(n):
        d = int.from_bytes(sk[i].tobytes(), "big"); kk = int.from_bytes(k[i].tobytes(), "big")
        if Pk[i, 63] & 1: d = N - d
        if R[i, 63] & 1: kk = N - kk
        rx, px = R[i, :32].tobytes(), Pk[i, :32].tobytes()
        e = int.from_bytes(hashlib.sha256(tag + rx + px + msgs[i].tobytes()).digest(), "big") % N
        sigs[i, :32] = np.frombuffer(rx, np.uint8); sigs[i, 32:] = np.frombuffer(((kk + e * d) % N).to_bytes(32, "big"), np.uint8)
    return sigs, msgs, np.ascontiguousarray(Pk[:, :32])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigs", type=int, default=1 << 16)
    ap.add_argument("--agg-sizes", type=int, nargs="+", default=[2, 16, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(45)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    L, h = eng._lib, eng._h
    n = a.sigs
    sigs, msgs, keys = make_signatures(eng, rng, n)
    d_sig, d_msg, d_key = (torch.from_numpy(v).to(dev) for v in (sigs, msgs, keys))
    d_v = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.schnorrsig_verify_batch_dev(d_v, d_sig, d_msg, d_key); eng.sync()
    assert bool(d_v.all()), "a signature made here does not verify"

    def ok(r, what):
        if not r:
            raise RuntimeError(what + ": " + _native.last_error())

    def wall(call):
        t = time.perf_counter(); call(); eng.sync()
        return (time.perf_counter() - t) * 1e3

    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "signatures": n,
           "timing": "wall-clock ms, call to s2k_engine_sync; chain_kernel_ms: s2k_engine_last_ms(1) of the aggregation call", "aggregate_sizes": {}}
    calls = {"verify_unaggregated": (lambda: eng.schnorrsig_verify_batch_dev(d_v, d_sig, d_msg, d_key), n)}
    chain_ms, checks = {}, []
    for m in a.agg_sizes:
        K = n // m; ns = K * m
        item_off = np.arange(0, ns + 1, m, dtype=np.uint64); agg_off = np.array([32 * (int(item_off[k]) + k) for k in range(K + 1)], np.uint64)
        d_made = torch.zeros(K, dtype=torch.int32, device=dev); d_res = torch.zeros(K, dtype=torch.int32, device=dev); d_agg = torch.zeros(32 * (ns + K), dtype=torch.uint8, device=dev)
        KL = min(K, a.loop_max)
        d_resl = torch.zeros(KL, dtype=torch.int32, device=dev); d_resb = torch.zeros(KL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def aggregate(m=m, K=K, item_off=item_off, d_made=d_made, d_agg=d_agg):
            ok(L.secp256k1_schnorrsig_aggregate_batch_dev(h, None, _dp(d_made), _dp(d_agg), _dp(d_key), 0, _dp(d_msg), _dp(d_sig), _p(item_off), K), "aggregate_batch_dev")

        def verify(K=K, item_off=item_off, agg_off=agg_off, d_res=d_res, d_agg=d_agg):
            ok(L.secp256k1_schnorrsig_aggverify_batch_dev(h, None, _dp(d_res), _dp(d_key), 0, _dp(d_msg), _p(item_off), _dp(d_agg), _p(agg_off), K), "aggverify_batch_dev")

        def verify_first(KL=KL, item_off=item_off, agg_off=agg_off, d_resb=d_resb, d_agg=d_agg):
            ok(L.secp256k1_schnorrsig_aggverify_batch_dev(h, None, _dp(d_resb), _dp(d_key), 0, _dp(d_msg), _p(item_off), _dp(d_agg), _p(agg_off), KL), "aggverify_batch_dev")

        def loop(m=m, KL=KL, d_resl=d_resl, d_agg=d_agg):
            for k in range(KL):
                ok(L.secp256k1_schnorrsig_aggverify_dev(h, None, ctypes_ptr(d_resl, 4 * k), ctypes_ptr(d_key, 32 * m * k), 0, ctypes_ptr(d_msg, 32 * m * k), m,
                                                        ctypes_ptr(d_agg, 32 * (m * k + k)), 32 * (m + 1)), "aggverify_dev")
        calls["aggregate_batch_%d" % m] = (aggregate, ns)
        calls["aggverify_batch_%d" % m] = (verify, ns)
        calls["aggverify_batch_first_%d_of_%d" % (KL, m)] = (verify_first, KL * m)
        calls["single_loop_first_%d_of_%d" % (KL, m)] = (loop, KL * m)
        checks.append((m, d_made, d_res, d_resb, d_resl))
        chain_ms[m] = []
    for _ in range(2):
        for name, (call, items) in calls.items():
            call(); eng.sync()
    for m, d_made, d_res, d_resb, d_resl in checks:
        assert bool(d_made.all()) and bool(d_res.all()) and bool(d_resb.all()) and bool(d_resl.all()), "size %d: an aggregate was refused" % m
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for name, (call, items) in calls.items():
            ms[name].append(wall(call))
            if name.startswith("aggregate_batch_"):
                chain_ms[int(name.rsplit("_", 1)[1])].append(eng.last_ms(1))
    rows = {k: stats(ms[k], calls[k][1]) for k in calls}
    out["verify_unaggregated"] = rows.pop("verify_unaggregated")
    failed = []
    for m in a.agg_sizes:
        K = n // m; KL = min(K, a.loop_max)
        row = {"aggregates": K, "aggregate_batch": rows["aggregate_batch_%d" % m], "aggverify_batch": rows["aggverify_batch_%d" % m],
               "first_%d" % KL: {"aggverify_batch": rows["aggverify_batch_first_%d_of_%d" % (KL, m)], "single_loop": rows["single_loop_first_%d_of_%d" % (KL, m)]}}
        for k in ("aggregate_batch", "aggverify_batch"):
            row[k]["aggregates_per_s"] = round(K / row[k]["ms_median"] * 1e3, 1)
        c = sorted(chain_ms[m])[len(chain_ms[m]) // 2]
        row["chain_kernel_ms"] = round(c, 4)
        row["chain_share_of_aggverify_batch"] = round(c / row["aggverify_batch"]["ms_median"], 3)
        row["chain_share_of_aggregate_batch"] = round(c / row["aggregate_batch"]["ms_median"], 3)
        f = row["first_%d" % KL]
        f["loop_over_batch"] = round(f["single_loop"]["ms_median"] / f["aggverify_batch"]["ms_median"], 2)
        f["ranges_clear"] = bool(f["aggverify_batch"]["ms_max"] < f["single_loop"]["ms_min"])
        if m == 16 and KL == 256 and not f["ranges_clear"]:
            failed.append("256 aggregates of 16: batch %.3f..%.3f ms, loop %.3f..%.3f ms" % (f["aggverify_batch"]["ms_min"], f["aggverify_batch"]["ms_max"],
                                                                                               f["single_loop"]["ms_min"], f["single_loop"]["ms_max"]))
        out["aggregate_sizes"][str(m)] = row
    out["condition_256_aggregates_of_16_batch_faster_than_loop"] = (not failed) if any(m == 16 for m in a.agg_sizes) else "not run"
    eng.close()
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        print("CONDITION MISSED: " + "; ".join(failed), file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
