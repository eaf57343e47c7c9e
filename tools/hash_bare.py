#!/usr/bin/env python3
"""Device-resident timing of the hash calls (csrc/engine_hash.hip) next to secp256k1_ecdsa_verify_batch_dev, in one process, at the same n:

    python tools/hash_bare.py [--sizes 65536 1048576] [--rounds 7] [--out profiles/hash_rates.json]

    fixed lengths 32, 64, 200 and 1 000 bytes (the msglen form) and one mixed batch (lengths uniform in 100 .. 300, the msg_off form),
    each as SHA256, SHA256 of SHA256 and a tagged hash; and a 200-byte batch of as many items as give the mixed batch's number of
    compressions (what the mixed batch would cost if no wavefront waited for its longest message).

Times are the HIP events the engine records around a call's launches (s2k_engine_last_ms(0)).  After two warm-up calls of each, every hash
call alternates with the ECDSA call for --rounds rounds; every figure is the median of the rounds with their minimum and maximum.
Recorded per shape: items/s, compressions/s, the fraction of the derived ceiling (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz / 1 709
instructions per compression), the ratio of a hashed item's time to an ECDSA-verified item's, and hashlib.sha256 on one core of this box
over the first 65 536 items.

Inputs.  One buffer of random bytes serves every shape.  The ECDSA items are n distinct valid signatures by n distinct keys (nonce points
and keys by the engine's own s2k_ecmult_batch, s by integer arithmetic); every one must verify.  The first and last digests of every
shape are compared with hashlib."""
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

CEILING = 256 * 4 * 16 * 2.4e9 / 1709          # compressions/s: one VALU instruction per lane and cycle, nothing but the 1 709 of a block (sha256.h's own count)
BLOCK_VALU = 1386                              # VALU instructions of one pass of k_hash_batch<0>'s block loop in the compiler's assembly: fewer than 1 709
CEILING_AS_BUILT = 256 * 4 * 16 * 2.4e9 / BLOCK_VALU
TAG = b"TapSighash"
FIXED = (32, 64, 200, 1000)
MODES = ("sha256", "sha256d", "tagged")
CPU_ITEMS = 1 << 16
TAG_PREFIX = hashlib.sha256(TAG).digest() * 2


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def compact(obj):
    """JSON with one line per innermost object or list"""
    flat = lambda m: re.sub(r"\s*\n\s*", " ", m.group(0))      # noqa: E731
    return re.sub(r"\{[^{}\[\]]*\}|\[[^{}\[\]]*\]", flat, json.dumps(obj, indent=1))


def blocks(length, mode):
    """compressions of one item: the message with its padding, one more for the second round (the tag's prefix is in the start state)"""
    return (int(length) + 9 + 63) // 64 + (1 if mode == "sha256d" else 0)


def digest(mode, m):
    if mode == "sha256":
        return hashlib.sha256(m).digest()
    if mode == "sha256d":
        return hashlib.sha256(hashlib.sha256(m).digest()).digest()
    return hashlib.sha256(TAG_PREFIX + m).digest()


def batch_inverse(vals):
    pre, run = [], 1
    for v in vals:
        pre.append(run); run = run * v % N
    inv = pow(run, -1, N)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % N; inv = inv * vals[i] % N
    return out


def make_ecdsa(eng, n, rng):
    """n valid signatures: compact sigs (n,64), msghash (n,32), compressed keys (n,33)"""
    def scalars():
        a = rng.integers(0, 256, (n, 32), dtype=np.uint8); a[:, 0] &= 0x3F; a[:, 31] |= 1
        return a
    ints = lambda a: [int.from_bytes(r.tobytes(), "big") for r in a]      # noqa: E731
    d, k = scalars(), scalars()
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    g = np.tile(np.frombuffer(G_XY, np.uint8), (n, 1)); zero = np.zeros((n, 32), np.uint8)
    X = eng.ecmult_batch(g, zero, ng=d)[0]; R = eng.ecmult_batch(g, zero, ng=k)[0]
    pk = np.concatenate([(2 + (X[:, 63] & 1))[:, None], X[:, :32]], axis=1).astype(np.uint8)
    di, ki, mi = ints(d), ints(k), ints(msg)
    kinv = batch_inverse(ki)
    sig = bytearray()
    for i in range(n):
        r = int.from_bytes(R[i, :32].tobytes(), "big") % N
        s = (mi[i] % N + r * di[i]) * kinv[i] % N
        s = min(s, N - s)
        sig += r.to_bytes(32, "big") + s.to_bytes(32, "big")
    return np.frombuffer(bytes(sig), np.uint8).reshape(n, 64), msg, pk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(46)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    nmax = max(a.sizes)
    data = rng.integers(0, 256, nmax * max(FIXED), dtype=np.uint8)
    d_data = torch.from_numpy(data).to(dev)
    sig, emsg, pk = make_ecdsa(eng, nmax, rng)
    d_sig, d_emsg, d_pk = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (sig, emsg, pk))
    out = {"so_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest(), "src_sha256": _native.sources_sha256(),
           "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "timing": "s2k_engine_last_ms(0): the events around a call's launches (the zeroing of the output included)", "tag": TAG.decode(),
           "ceiling_compressions_per_s": round(CEILING, 1), "ceiling": "derived: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz / 1 709 instructions",
           "ceiling_as_built_compressions_per_s": round(CEILING_AS_BUILT, 1), "ceiling_as_built": "the same with the %d VALU instructions the block loop has in this build's assembly" % BLOCK_VALU, "sizes": {}}
    for n in a.sizes:
        res = torch.zeros(n, dtype=torch.int32, device=dev)
        dig = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        lens = rng.integers(100, 301, n)
        off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
        d_off = torch.from_numpy(off).to(dev)
        shapes = {("fixed_%d" % ln): (ln, None, n) for ln in FIXED}
        shapes["mixed_100_300"] = (None, lens, n)

        def call(mode, ln, items, offs=None):
            kw = dict(msglen=ln, n=items) if offs is None else dict(msg_off=offs, n=items)
            if mode == "tagged":
                eng.tagged_sha256_batch_dev(dig, TAG, d_data, **kw)
            else:
                eng.sha256_batch_dev(dig, d_data, rounds=2 if mode == "sha256d" else 1, **kw)
        ecdsa = lambda: eng.ecdsa_verify_batch_dev(res, d_sig[:n], d_emsg[:n], d_pk[:n], n=n)      # noqa: E731
        calls = {}
        for name, (ln, ls, items) in shapes.items():
            for mode in MODES:
                comps = items * blocks(ln, mode) if ls is None else int(sum(blocks(v, mode) for v in ls))
                calls[(name, mode)] = ((lambda mode=mode, ln=ln, items=items, ls=ls: call(mode, ln, items, None if ls is None else d_off)), items, comps)
        for mode in MODES:                           # the mixed batch's compressions as 200-byte items
            comps = calls[("mixed_100_300", mode)][2]
            items = comps // blocks(200, mode)
            assert items <= n
            calls[("fixed_200_same_compressions_as_mixed", mode)] = ((lambda mode=mode, items=items: call(mode, 200, items)), items, items * blocks(200, mode))
        # warm-up, with a check of the first and the last digest of every shape
        for w in range(2):
            for (name, mode), (fn, items, comps) in calls.items():
                fn(); eng.sync()
                if w == 0 and items <= n:
                    got = dig[:items].cpu().numpy()
                    ln, ls, _ = shapes.get(name, (200, None, items))
                    for i in (0, items - 1):
                        lo, hi = (i * ln, (i + 1) * ln) if ls is None else (int(off[i]), int(off[i + 1]))
                        assert got[i].tobytes() == digest(mode, data[lo:hi].tobytes()), (name, mode, i)
            ecdsa(); eng.sync()
            assert bool(res.all()), "an ECDSA item was refused"
        ms = {k: [] for k in calls}; ems = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, (fn, items, comps) in calls.items():
                fn(); eng.sync(); ms[k].append(eng.last_ms(0))
                ecdsa(); eng.sync(); ems[k].append(eng.last_ms(0))
        row = {}
        all_e = sorted(v for vs in ems.values() for v in vs)
        row["ecdsa_verify"] = stats(all_e, n)
        row["ecdsa_verify"]["calls"] = len(all_e)
        for (name, mode), (fn, items, comps) in calls.items():
            st = stats(ms[(name, mode)], items)
            st["items"] = items; st["compressions"] = comps
            st["compressions_per_s"] = round(comps / st["ms_median"] * 1e3, 1)
            st["fraction_of_ceiling"] = round(st["compressions_per_s"] / CEILING, 4)
            st["fraction_of_ceiling_as_built"] = round(st["compressions_per_s"] / CEILING_AS_BUILT, 4)
            e_med = sorted(ems[(name, mode)])[len(ems[(name, mode)]) // 2]
            st["item_time_over_ecdsa_item_time"] = round((st["ms_median"] / items) / (e_med / n), 5)
            row.setdefault(name, {})[mode] = st
        row["mixed_over_fixed_with_same_compressions"] = {
            mode: round(row["mixed_100_300"][mode]["ms_median"] / row["fixed_200_same_compressions_as_mixed"][mode]["ms_median"], 3) for mode in MODES}
        # hashlib on one core over the first CPU_ITEMS items of every shape of this n
        cpu = {}
        m = min(n, CPU_ITEMS)
        for name, (ln, ls, items) in shapes.items():
            msgs = [data[i * ln:(i + 1) * ln].tobytes() for i in range(m)] if ls is None else [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(m)]
            for mode in MODES:
                t0 = time.perf_counter()
                for x in msgs:
                    digest(mode, x)
                dt = time.perf_counter() - t0
                cpu.setdefault(name, {})[mode] = {"items": m, "items_per_s": round(m / dt, 1), "gpu_over_cpu": round(row[name][mode]["items_per_s"] / (m / dt), 1)}
        row["hashlib_one_core"] = cpu
        out["sizes"][str(n)] = row
    eng.close()
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
