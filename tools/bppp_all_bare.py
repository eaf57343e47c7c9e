#!/usr/bin/env python3
"""Device-resident timing of the one-verdict BP++ norm-argument verifier next to the per-item verifier, in one process over the same buffers:

    python tools/bppp_all_bare.py [--sizes 256 1024 4096 16384 65536] [--rounds 7] [--g-len 64] [--h-len 8] [--out profiles/bppp_all_rates.json]

Per size n (all proofs valid, every array in HBM, the generator set's fixed-base table built before anything is timed):
  verify_all   secp256k1_bppp_norm_product_verify_all_dev: one verdict (asserted to be 1 after every round)
  per_item     secp256k1_bppp_norm_product_verify_batch_dev: n verdicts
The two calls alternate for --rounds rounds (at least five) after two warm-up calls of each.  Times are wall-clock milliseconds from
before the call to after s2k_engine_sync; the call's own span between its device events (s2k_engine_last_ms(0)) stands beside it.  Every
figure is the median with the minimum and maximum.  The split of verify_all is taken from its events after every round
(s2k_bppp_all_last_split_ms): per-proof scalars and item digests / hash tree, seed and z' / column sums and own terms / multi-scalar
multiplication.  `crossover_n` is the smallest measured n at which verify_all's slowest round beats the per-item call's fastest round
(null: none did); `crossover_n_sustained` the smallest one from which that holds at every larger measured size too.

The proofs come from the reference's prover (oracle/_ref through tests/refapi.py): --distinct of them (default 256), repeated up to the
largest size, as tests/test_gpu_bppp.py::test_config4_full_size does; every proof is checked by the per-item verifier before anything
is timed.  There is no CPU path: without a GPU this fails."""
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

PHASES = ["scalars_and_item_digests_ms", "tree_seed_and_coefficients_ms", "column_sums_and_own_terms_ms", "msm_ms"]


def stats(ms, items=None):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    out = {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
    if items:
        out["spread_pct"] = round(100 * (ms[-1] - ms[0]) / med, 2)
        out["proofs_per_s"] = round(items / med * 1e3, 1)
    return out


def compact(obj):
    flat = lambda m: re.sub(r"\s*\n\s*", " ", m.group(0))      # noqa: E731
    return re.sub(r"\{[^{}\[\]]*\}|\[[^{}\[\]]*\]", flat, json.dumps(obj, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--g-len", type=int, default=64)
    ap.add_argument("--h-len", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bppp_all_bare: no GPU (there is no CPU path to time)")
    from tests import refapi
    sizes = sorted(set(a.sizes))
    nmax = sizes[-1]
    base = refapi.Ref().make_bppp(min(a.distinct, nmax), np.random.default_rng(412), a.g_len, a.h_len)
    reps = (nmax + base[2].shape[0] - 1) // base[2].shape[0]
    proofs, trs, rhos, cvs, commits = (np.ascontiguousarray(np.concatenate([base[k]] * reps)[:nmax]) for k in (0, 1, 2, 5, 6))
    gens, g_len = np.ascontiguousarray(base[3]), base[4]
    proof_len, h_len = proofs.shape[1], cvs.shape[1]
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    d_p, d_t, d_r, d_g, d_c, d_m = (torch.from_numpy(v).to(dev) for v in (proofs, trs, rhos, gens, cvs, commits))
    d_res = torch.zeros(nmax, dtype=torch.int32, device=dev); d_v = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.bppp_norm_product_verify_batch_dev(d_res, d_p, proof_len, d_t, d_r, d_g, gens, g_len, d_c, h_len, d_m, nmax); eng.sync()      # (builds the set's table)
    assert bool(d_res.all()), "a proof made here does not verify"

    def wall(call):
        t = time.perf_counter(); call(); eng.sync()
        return (time.perf_counter() - t) * 1e3

    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmups": 2, "g_len": g_len, "h_len": h_len, "proof_len": proof_len,
           "distinct_proofs": int(base[2].shape[0]),
           "timing": "wall: wall-clock ms, call to s2k_engine_sync; events: s2k_engine_last_ms(0); split: s2k_bppp_all_last_split_ms; the two calls alternate", "sizes": {}}
    crossover = None
    for n in sizes:
        r = d_res[:n]

        def verify_all():
            eng.bppp_norm_product_verify_all_dev(d_v, d_p, proof_len, d_t, d_r, d_g, gens, g_len, d_c, h_len, d_m, n)

        def per_item():
            eng.bppp_norm_product_verify_batch_dev(r, d_p, proof_len, d_t, d_r, d_g, gens, g_len, d_c, h_len, d_m, n)
        for _ in range(2):
            verify_all(); eng.sync(); per_item(); eng.sync()
        w = {"verify_all": [], "per_item": []}; ev = {"verify_all": [], "per_item": []}; split = [[] for _ in PHASES]
        for _ in range(a.rounds):
            d_v.zero_(); torch.cuda.synchronize()
            w["verify_all"].append(wall(verify_all)); ev["verify_all"].append(eng.last_ms(0))
            for q, x in enumerate(eng.bppp_all_last_split_ms()):
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
