#!/usr/bin/env python3
"""Device-resident timing of the one-verdict BIP-340 batch verifier next to the per-item verifier, in one process over the same buffers:

    python tools/schnorr_all_bare.py [--sizes 4096 16384 65536 262144 1048576] [--rounds 5] [--out profiles/schnorr_all_rates.json]

Per size n (the first n of the signatures made for the largest size; all valid, every array in HBM):
  verify_all   secp256k1_schnorrsig_verify_all_dev: one verdict (asserted to be 1 after every round)
  per_item     secp256k1_schnorrsig_verify_batch_dev: n verdicts
The two calls alternate for --rounds rounds (at least five) after two warm-up calls of each.  Times are wall-clock milliseconds from
before the call to after s2k_engine_sync; the call's own span between its device events (s2k_engine_last_ms(0)) stands beside it.  Every
figure is the median with the minimum and maximum.  The split of verify_all is taken from its events after every round
(s2k_schnorr_all_last_split_ms): lift and item hashes / hash tree and seed / coefficients and scalar sum / multi-scalar multiplication.
`crossover_n` is the smallest measured n at which verify_all's slowest round beats the per-item call's fastest round (null: none did);
`crossover_n_sustained` the smallest one from which that holds at every larger measured size too.

Signatures are made here (BIP-340 with public test keys: the engine's s2k_ecmult_batch gives x_i G and k_i G, Python the challenges and
s_i); every signature is checked by the per-item verifier before anything is timed.  There is no CPU path: without a GPU this fails."""
import argparse
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
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402

PHASES = ["lift_and_item_hashes_ms", "tree_and_seed_ms", "coefficients_and_scalar_sum_ms", "msm_ms"]


def stats(ms, items=None):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    out = {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
    if items:
        out["spread_pct"] = round(100 * (ms[-1] - ms[0]) / med, 2)
        out["signatures_per_s"] = round(items / med * 1e3, 1)
    return out


def compact(obj):
    flat = lambda m: re.sub(r"\s*\n\s*", " ", m.group(0))      # noqa: E731
    return re.sub(r"\{[^{}\[\]]*\}|\[[^{}\[\]]*\]", flat, json.dumps(obj, indent=1))


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
    skb, kb, Pb, Rb, mb = sk.tobytes(), k.tobytes(), Pk.tobytes(), R.tobytes(), msgs.tobytes()
    out = bytearray(64 * n)
    for i in range(n):
        d = int.from_bytes(skb[32 * i:32 * i + 32], "big"); kk = int.from_bytes(kb[32 * i:32 * i + 32], "big")
        if Pb[64 * i + 63] & 1: d = N - d
        if Rb[64 * i + 63] & 1: kk = N - kk
        rx, px = Rb[64 * i:64 * i + 32], Pb[64 * i:64 * i + 32]
        e = int.from_bytes(hashlib.sha256(tag + rx + px + mb[32 * i:32 * i + 32]).digest(), "big") % N
        out[64 * i:64 * i + 32] = rx; out[64 * i + 32:64 * i + 64] = ((kk + e * d) % N).to_bytes(32, "big")
    sigs = np.frombuffer(bytes(out), np.uint8).reshape(n, 64).copy()
    return sigs, msgs, np.ascontiguousarray(Pk[:, :32])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("schnorr_all_bare: no GPU (there is no CPU path to time)")
    sizes = sorted(set(a.sizes))
    rng = np.random.default_rng(340)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    nmax = sizes[-1]
    sigs, msgs, keys = make_signatures(eng, rng, nmax)
    d_sig, d_msg, d_key = (torch.from_numpy(v).to(dev) for v in (sigs, msgs, keys))
    d_res = torch.zeros(nmax, dtype=torch.int32, device=dev); d_v = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.schnorrsig_verify_batch_dev(d_res, d_sig, d_msg, d_key); eng.sync()
    assert bool(d_res.all()), "a signature made here does not verify"

    def wall(call):
        t = time.perf_counter(); call(); eng.sync()
        return (time.perf_counter() - t) * 1e3

    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmups": 2, "msglen": 32, "pk_format": 0,
           "timing": "wall: wall-clock ms, call to s2k_engine_sync; events: s2k_engine_last_ms(0); split: s2k_schnorr_all_last_split_ms; the two calls alternate", "sizes": {}}
    crossover = None
    for n in sizes:
        s, m, k, r = d_sig[:n], d_msg[:n], d_key[:n], d_res[:n]

        def verify_all():
            eng.schnorrsig_verify_all_dev(d_v, s, m, k, n=n)

        def per_item():
            eng.schnorrsig_verify_batch_dev(r, s, m, k)
        for _ in range(2):
            verify_all(); eng.sync(); per_item(); eng.sync()
        w = {"verify_all": [], "per_item": []}; ev = {"verify_all": [], "per_item": []}; split = [[] for _ in PHASES]
        for _ in range(a.rounds):
            d_v.zero_(); torch.cuda.synchronize()
            w["verify_all"].append(wall(verify_all)); ev["verify_all"].append(eng.last_ms(0))
            for q, x in enumerate(eng.schnorr_all_last_split_ms()):
                split[q].append(x)
            assert int(d_v.cpu()[0]) == 1, "verify_all refused a valid batch of %d" % n
            w["per_item"].append(wall(per_item)); ev["per_item"].append(eng.last_ms(0))
        assert bool(r.all())
        row = {name: {"wall": stats(w[name], n), "events": stats(ev[name], n)} for name in w}
        row["split_of_verify_all"] = {PHASES[q]: stats(split[q]) for q in range(len(PHASES))}
        row["per_item_over_verify_all"] = {"median": round(row["per_item"]["wall"]["ms_median"] / row["verify_all"]["wall"]["ms_median"], 3),
                                           "lowest": round(row["per_item"]["wall"]["ms_min"] / row["verify_all"]["wall"]["ms_max"], 3),
                                           "highest": round(row["per_item"]["wall"]["ms_max"] / row["verify_all"]["wall"]["ms_min"], 3)}
        row["ranges_clear"] = bool(row["verify_all"]["wall"]["ms_max"] < row["per_item"]["wall"]["ms_min"])
        if row["ranges_clear"] and crossover is None:
            crossover = n
        out["sizes"][str(n)] = row
    out["crossover_n"] = crossover
    sustained = None
    for n in reversed(sizes):
        if not out["sizes"][str(n)]["ranges_clear"]:
            break
        sustained = n
    out["crossover_n_sustained"] = sustained
    eng.close()
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
