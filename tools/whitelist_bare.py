#!/usr/bin/env python3
"""Device-resident timing of whitelist-signature verification (k_wl_keys + k_wl_ring) through secp256k1_whitelist_verify_batch_dev, next to
k_ecdsa_verify (secp256k1_ecdsa_verify_batch_dev) in the same process, on the same box, at the same number of lanes as the ring kernel
(n), and the reference's secp256k1_whitelist_verify on one core through ctypes on a bounded sample:

    python tools/whitelist_bare.py --n 65536 --keys 15 [--reps 5] [--out profiles/whitelist_rates.json]      (--out appends a row)

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(0): both kernels; (1): k_wl_ring alone), after two
warm-up calls; every figure is the median of --reps calls with their minimum and maximum beside it.

Inputs.  ONE whitelist of --keys keys for the whole batch (list_of names list 0 for every item: the usual case).  The first 64 items are
reference-made and must verify (checked).  The rest do the same work without costing a CPU signature each: a valid sub key, a random e0
and random s_j below the group order run every key lane and every ring position and are refused only by the final comparison."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from tests.ecdsa_ref import EcdsaRef  # noqa: E402
from tests.whitelist_ref import Whitelist, WhitelistRef  # noqa: E402

NV = 64          # reference-made items
NSUB = 4096      # distinct sub keys of the filler items


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2)}


def timed(eng, call, reps, which):
    for _ in range(2):
        call()
    eng.sync()
    out = [[] for _ in which]
    for _ in range(reps):
        call(); eng.sync()
        for o, w in zip(out, which):
            o.append(eng.last_ms(w))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--keys", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-sample", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.n < NV or not 1 <= a.keys <= 255:
        ap.error(f"--n at least {NV}, --keys 1..255")
    n, K = a.n, a.keys
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(41)
    wr = WhitelistRef(); er = EcdsaRef()
    w = Whitelist(wr, rng, K)
    on, off = b"".join(w.online), b"".join(w.offline)
    slen = 33 + 32 * K
    sigs = rng.integers(0, 256, (n, slen), dtype=np.uint8)
    sigs[:, 0] = K
    sigs[:, 33::32] &= 0x7F                                          # every s_j below the group order
    pool = np.frombuffer(b"".join(wr.pubkey_create(bytes(rng.integers(0, 256, 31, dtype=np.uint8).tolist()) + b"\x01") for _ in range(NSUB)), np.uint8).reshape(NSUB, 64)
    subs = np.tile(pool, ((n + NSUB - 1) // NSUB, 1))[:n].copy()
    valid = []
    for i in range(NV):
        s, sub = w.sign(wr, rng, i % K)
        sigs[i] = np.frombuffer(s, np.uint8); subs[i] = np.frombuffer(sub, np.uint8)
        valid.append((s, sub))
    t0 = time.perf_counter()
    for s, sub in valid[:a.cpu_sample]:
        assert wr.verify(s, on, off, sub) == 1
    cpu_ms = (time.perf_counter() - t0) * 1e3 / a.cpu_sample
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    d_sig, d_sub, d_on, d_off = T(sigs.reshape(-1)), T(subs.reshape(-1)), T(np.frombuffer(on, np.uint8)), T(np.frombuffer(off, np.uint8))
    sig_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(slen); list_off = np.array([0, K], np.uint64); list_of = np.zeros(n, np.uint32)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    eng = Engine(0)
    both, ring = timed(eng, lambda: eng.whitelist_verify_batch_dev(res, d_sig, sig_off, d_on, d_off, list_off, d_sub, list_of=list_of), a.reps, (0, 1))
    got = res.cpu().numpy()
    assert got[:NV].all() and not got[NV:].any(), "whitelist: wrong verdicts"
    # k_ecdsa_verify at n lanes: reference-made signatures tiled over random hashes' worth of work (random r, low s, valid keys)
    d = er.make(256, rng)
    e_sig = rng.integers(0, 256, (n, 64), dtype=np.uint8); e_sig[:, 0] &= 0x7F; e_sig[:, 32] &= 0x3F
    e_msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    e_pk = np.tile(er.pks_as(d["pkobj"], 0), ((n + 255) // 256, 1))[:n]
    de = [T(e_sig), T(e_msg), T(e_pk)]
    (ems,) = timed(eng, lambda: eng.ecdsa_verify_batch_dev(res, de[0], de[1], de[2], n=n), a.reps, (1,))
    eng.close()
    tb, tr, te = stats(both), stats(ring), stats(ems)
    row = {"n": n, "keys_per_list": K, "so_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest(), "src_sha256": _native.sources_sha256(),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "reference_made_items": NV,
           "whitelist_both_kernels": tb, "k_wl_ring": tr, "k_wl_keys_ms_median": round(tb["ms_median"] - tr["ms_median"], 4),
           "signatures_per_s": round(n / tb["ms_median"] * 1e3, 1), "keys_per_s": round(n * K / tb["ms_median"] * 1e3, 1),
           "ecdsa_verify_same_lanes": te, "ecdsa_verifies_per_s": round(n / te["ms_median"] * 1e3, 1),
           "reference_cpu_one_core": {"sample": a.cpu_sample, "ms_per_signature": round(cpu_ms, 4), "signatures_per_s": round(1e3 / cpu_ms, 2), "keys_per_s": round(K * 1e3 / cpu_ms, 1)}}
    row["keys_per_s_over_ecdsa"] = round(row["keys_per_s"] / row["ecdsa_verifies_per_s"], 4)
    text = json.dumps(row, indent=1)
    print(text)
    if a.out:
        rows = json.load(open(a.out)) if os.path.exists(a.out) else []
        rows.append(row)
        with open(a.out, "w") as f:
            f.write(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
