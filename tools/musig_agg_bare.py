#!/usr/bin/env python3
"""Device-resident timing of MuSig2 key aggregation (secp256k1_musig_pubkey_agg_batch_dev) next to its two yardsticks in the same
process over the same keys, and of the cache tweaks, nonce aggregation and signature aggregation:

    python tools/musig_agg_bare.py [--sizes 65536 1048576] [--set-sizes 2 16 256] [--rounds 3] [--out profiles/musig_agg_rates.json]

Yardsticks: s2k_ecmult_batch_dev with ng = NULL and random na -- one variable-base multiplication per key, the work of stage (b) --
and s2k_ecmult_multi_many_dev over the same sets with coefficients made beforehand (random 256-bit scalars, 1 for each set's second
key): what a caller could do before this call existed, its hashing not counted.

Times are the HIP events the engine records around a call's launches (s2k_engine_last_ms(0): the whole chain; for key aggregation also
last_ms(1): stage (b) alone).  After two warm-up calls of each, the calls alternate for --rounds rounds; every figure is the median of
the rounds with their minimum and maximum (the spread) beside it.

Inputs.  The keys are n distinct points x_i G made by the engine's own s2k_ecmult_batch; every set is served, and the cache of the
first set of every shape is compared with a Python computation (hashlib and integers).  Tweaks run on the caches the 2-key sets gave
(repeated to n items), x-only and plain alternating; nonce aggregation takes the keys pairwise as pubnonce objects in sessions of 2 and
of 16; signature aggregation sums random shares in sessions of 2 and of 16 under sessions that carry the magic and random bytes."""
import argparse
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
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402

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


def tagged(tag, data):
    t = hashlib.sha256(tag).digest()
    return hashlib.sha256(t + t + data).digest()


def _add(a, b):
    """affine addition over integers (None: infinity)"""
    if a is None or b is None:
        return b if a is None else a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P_FIELD == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P_FIELD) % P_FIELD
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P_FIELD) % P_FIELD
    x = (lam * lam - a[0] - b[0]) % P_FIELD
    return x, (lam * (a[0] - x) - a[1]) % P_FIELD


def _mul(k, a):
    r = None
    while k:
        if k & 1:
            r = _add(r, a)
        a = _add(a, a); k >>= 1
    return r


def expected_cache(keys_xy):
    """the cache of a set of distinct points given as 64 big-endian bytes each"""
    pts = [(int.from_bytes(k[:32].tobytes(), "big"), int.from_bytes(k[32:].tobytes(), "big")) for k in keys_xy]
    ser = [bytes([2 + (p[1] & 1)]) + p[0].to_bytes(32, "big") for p in pts]
    h = tagged(b"KeyAgg list", b"".join(ser))
    Q = None
    for i, p in enumerate(pts):
        Q = _add(Q, p if i == 1 else _mul(int.from_bytes(tagged(b"KeyAgg coefficient", h + ser[i]), "big") % N, p))
    le = lambda v: v.to_bytes(32, "little")      # noqa: E731
    second = le(pts[1][0]) + le(pts[1][1]) if len(pts) > 1 else bytes(64)
    return bytes([0xf4, 0xad, 0xbb, 0xdf]) + le(Q[0]) + le(Q[1]) + second + h + bytes(33)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--set-sizes", type=int, nargs="+", default=[2, 16, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference-us", default=None, help="the reference's per-call times as tests/golden/make_musig_agg_golden.py --time printed them: recorded as given")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(44)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    nmax = max(a.sizes)

    def scalars(k):
        s = rng.integers(0, 256, (k, 32), dtype=np.uint8); s[:, 0] &= 0x7F; s[:, 31] |= 1      # in [1, 2^255): below n, nonzero
        return s
    X = eng.ecmult_batch(np.tile(np.frombuffer(G_XY, np.uint8), (nmax, 1)), np.zeros((nmax, 32), np.uint8), ng=scalars(nmax))[0]      # n x (x | y), big-endian
    ser = np.concatenate([(2 + (X[:, 63] & 1))[:, None], X[:, :32]], axis=1).astype(np.uint8)
    obj = np.ascontiguousarray(np.concatenate([X[:, 31::-1], X[:, :31:-1]], axis=1))
    coef = scalars(nmax)
    d_xy, d_ser, d_obj = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (X, ser, obj))
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "timing": "s2k_engine_last_ms(0), the whole launch chain of a call; stage_b: last_ms(1)", "sizes": {}}
    caches2, want_cache = None, {}
    for n in a.sizes:
        row = {}
        r_xy = torch.zeros((n, 64), dtype=torch.uint8, device=dev); r_inf = torch.zeros(n, dtype=torch.int32, device=dev)
        d_na = torch.from_numpy(coef[:n].copy()).to(dev)
        calls, check = {"ecmult_batch": (lambda: eng.ecmult_batch_dev(r_xy, r_inf, d_xy[:n], d_na), n, None)}, {}
        for m in a.set_sizes:
            if m > n:
                continue
            ns = n // m
            off = np.arange(0, ns * m + 1, m, dtype=np.uint64)
            res = torch.zeros(ns, dtype=torch.int32, device=dev); cache = torch.zeros((ns, 197), dtype=torch.uint8, device=dev); agg = torch.zeros((ns, 64), dtype=torch.uint8, device=dev)
            sc = coef[:ns * m].copy()
            if m > 1:
                sc[1::m] = 0; sc[1::m, 31] = 1
            d_sc = torch.from_numpy(sc).to(dev)
            mm_xy = torch.zeros((ns, 64), dtype=torch.uint8, device=dev); mm_inf = torch.zeros(ns, dtype=torch.int32, device=dev)
            for f, keys in ((0, d_ser), (1, d_obj)):
                name = "pubkey_agg_%dkey_format%d" % (m, f)
                calls[name] = ((lambda keys=keys, f=f, res=res, cache=cache, agg=agg, off=off, k=ns * m: eng.musig_pubkey_agg_dev(res, cache, agg, keys[:k], off, pk_format=f)), ns * m, ns)
                check[name] = (res, cache, m)
            calls["multi_many_%dkey" % m] = ((lambda mm_xy=mm_xy, mm_inf=mm_inf, d_sc=d_sc, off=off, k=ns * m: eng.ecmult_multi_many_dev(mm_xy, mm_inf, d_sc, d_xy[:k], off)), ns * m, ns)
        stage_b = {k: [] for k in check}
        for _ in range(2):
            for name, (call, items, sets) in calls.items():
                call(); eng.sync()
                if name in check:
                    res, cache, m = check[name]
                    assert bool(res.all()), name + ": a set was refused"
                    if m not in want_cache:
                        want_cache[m] = expected_cache(X[:m])
                    assert bytes(cache[0].cpu().numpy()) == want_cache[m], name + ": wrong cache"
                    if m == 2 and name.endswith("format0") and n == nmax:
                        caches2 = cache.clone()
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, (call, items, sets) in calls.items():
                call(); eng.sync(); ms[name].append(eng.last_ms(0))
                if name in stage_b:
                    stage_b[name].append(eng.last_ms(1))
        for name, (call, items, sets) in calls.items():
            row[name] = stats(ms[name], items)
            if sets is not None:
                row[name]["sets_per_s"] = round(sets / row[name]["ms_median"] * 1e3, 1)
            if name in stage_b:
                row[name]["stage_b_ms_median"] = round(sorted(stage_b[name])[len(stage_b[name]) // 2], 4)
        per = lambda k: row[k]["ms_median"] / calls[k][1]      # noqa: E731
        row["key_time_over_ecmult_batch_item_time"] = {k: round(per(k) / per("ecmult_batch"), 3) for k in check}
        row["key_time_over_multi_many_term_time"] = {k: round(per(k) / per("multi_many_%s" % k.split("_")[2]), 3) for k in check}
        out["sizes"][str(n)] = row
    # ---- the other three calls at the largest size
    n = nmax
    other = {}
    if caches2 is not None:
        reps = (n + caches2.shape[0] - 1) // caches2.shape[0]
        d_c = caches2.repeat(reps, 1)[:n].contiguous()
        d_t = torch.from_numpy(coef[:n].copy()).to(dev); d_xo = torch.from_numpy((np.arange(n) & 1).astype(np.uint8)).to(dev)
        res = torch.zeros(n, dtype=torch.int32, device=dev); oc = torch.zeros((n, 197), dtype=torch.uint8, device=dev); opk = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        other["pubkey_tweak_add"] = ((lambda: eng.musig_pubkey_tweak_add_dev(res, oc, opk, d_c, d_t, d_xo, n=n)), n, res)
    magic = np.frombuffer(bytes([0xf5, 0x7a, 0x3d, 0xa0]), np.uint8)
    nonces = np.concatenate([np.tile(magic, (n, 1)), obj[:n], np.roll(obj[:n], 1, axis=0)], axis=1)
    d_non = torch.from_numpy(np.ascontiguousarray(nonces)).to(dev)
    shares = scalars(n); d_sh = torch.from_numpy(shares).to(dev)
    for m in (2, 16):
        ns = n // m
        off = np.arange(0, ns * m + 1, m, dtype=np.uint64)
        res_n = torch.zeros(ns, dtype=torch.int32, device=dev); o_n = torch.zeros((ns, 66), dtype=torch.uint8, device=dev)
        other["nonce_agg_%d_per_session" % m] = ((lambda res_n=res_n, o_n=o_n, off=off, k=ns * m: eng.musig_nonce_agg_dev(res_n, o_n, d_non[:k], off, nonce_format=1, out_format=0)), ns * m, res_n)
        sess = rng.integers(0, 256, (ns, 133), dtype=np.uint8); sess[:, :4] = np.frombuffer(bytes([0x9d, 0xed, 0xe9, 0x17]), np.uint8)
        d_se = torch.from_numpy(sess).to(dev)
        res_s = torch.zeros(ns, dtype=torch.int32, device=dev); o_s = torch.zeros((ns, 64), dtype=torch.uint8, device=dev)
        other["partial_sig_agg_%d_per_session" % m] = ((lambda res_s=res_s, o_s=o_s, d_se=d_se, off=off, k=ns * m: eng.musig_partial_sig_agg_dev(res_s, o_s, d_se, d_sh[:k], off)), ns * m, res_s)
        if m == 2:
            want = (int.from_bytes(sess[0, 101:].tobytes(), "big") + int.from_bytes(shares[0].tobytes(), "big") + int.from_bytes(shares[1].tobytes(), "big")) % N
            sig_check = (o_s, want)
    for _ in range(2):
        for name, (call, items, res) in other.items():
            call(); eng.sync()
            assert bool(res.all()), name + ": an item was refused"
    assert int.from_bytes(bytes(sig_check[0][0, 32:].cpu().numpy()), "big") == sig_check[1], "partial_sig_agg: wrong sum"
    ms = {k: [] for k in other}
    for _ in range(a.rounds):
        for name, (call, items, res) in other.items():
            call(); eng.sync(); ms[name].append(eng.last_ms(0))
    out["other_calls_at_%d_items" % n] = {k: dict(stats(ms[k], other[k][1]), sessions_or_items=int(other[k][2].numel())) for k in other}
    eng.close()
    out["reference_cpu_us_per_call"] = a.reference_us or "not measured here: tests/golden/make_musig_agg_golden.py --time prints it where the reference's sources are"
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
