#!/usr/bin/env python3
"""Device-resident timing of k_ecdsa_verify and k_ecdsa_recover through the `_dev` entry points, next to k_schnorr_verify
(secp256k1_schnorrsig_verify_batch_dev) in the same process, on the same box, at the same n:

    python tools/ecdsa_bare.py [--sizes 65536 1048576] [--reps 7] [--out profiles/ecdsa_rates.json]
    S2K_LIB=<a -DS2K_ECDSA_DIAG_NO_SCINV build> python tools/ecdsa_bare.py ...       (tools/ecdsa_parts.py runs both and takes the difference)

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)), after two warm-up calls; every figure is the
median of --reps calls with their minimum and maximum beside it.

Inputs.  The first 2^14 items of every batch are reference-made and must all verify / recover to the signer's key (checked).  The rest do
the same work without costing a CPU signature each: a valid public key (or, for recovery, an r that lifts) with random r, low random s and
a random hash runs the whole item -- parsers, scalar inversion, the double multiplication with per-item scalars, the comparison -- and
is refused only by that last comparison.  Tiling the valid items instead would repeat every generator-table address 64 times."""
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
from tests.ecdsa_ref import EcdsaRef  # noqa: E402
from tests.refapi import Ref  # noqa: E402

NV = 1 << 14


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def timed(eng, call, reps):
    for _ in range(2):
        call()
    eng.sync()
    ms = []
    for _ in range(reps):
        call(); eng.sync()
        ms.append(eng.last_ms(1))
    return ms


def ref_cpu_figure():
    """the reference's own bench program on one core of this box (oracle/_ref/bench ecdsa_verify; bench.py builds it)"""
    b = os.path.join(ROOT, "oracle", "_ref", "bench")
    if not os.access(b, os.X_OK):
        return None
    out = subprocess.run([b, "ecdsa_verify"], env=dict(os.environ, SECP256K1_BENCH_ITERS="20000"), capture_output=True, text=True, timeout=120).stdout
    for line in out.splitlines():
        p = [x.strip() for x in line.split(",")]
        if len(p) == 4 and p[0] == "ecdsa_verify":
            mn, avg, mx = (float(x) for x in p[1:])
            return {"us_min_avg_max": [mn, avg, mx], "verifies_per_s_one_core": round(1e6 / avg, 1)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    er = EcdsaRef(); ref = Ref()
    nmax = max(max(a.sizes), NV)
    # reference-made part
    d = er.make(NV, rng)
    sig_v = er.sigs_as(d["sigobj"], 0); pk33_v = er.pks_as(d["pkobj"], 0)
    rmsg, rsig, rid, rpk = er.make_recoverable(NV, rng)
    ssig, smsg, spk = ref.make_schnorr(NV, rng, threads=16)

    def tiled(valid):                       # the NV valid rows repeated up to nmax rows (any nmax: rounded up, then cut)
        return np.tile(valid, ((nmax + NV - 1) // NV, 1))[:nmax]

    def fill(valid, width, rnd=True):
        out = rng.integers(0, 256, (nmax, width), dtype=np.uint8) if rnd else tiled(valid)
        out[:NV] = valid
        return out
    # ECDSA verify: random r, s with the top bit clear (low), random hashes, the valid keys tiled
    e_sig = fill(sig_v, 64); e_sig[NV:, 0] &= 0x7F; e_sig[NV:, 32] &= 0x3F
    e_msg = fill(d["msgs"], 32); e_pk = fill(pk33_v, 33, rnd=False)
    # recovery: r = the x coordinate of a valid key (it lifts), random low s, recid 0 / 1
    r_sig = fill(rsig, 64); r_sig[NV:, 0:32] = tiled(pk33_v[:, 1:])[NV:]; r_sig[NV:, 32] &= 0x3F
    r_msg = fill(rmsg, 32); r_id = np.concatenate([rid, rng.integers(0, 2, nmax - NV, dtype=np.uint8)])
    # BIP-340: random r below 2^255, random s below 2^255, the valid x-only keys tiled
    s_sig = fill(ssig, 64); s_sig[NV:, 0] &= 0x7F; s_sig[NV:, 32] &= 0x7F
    s_msg = fill(smsg, 32); s_pk = fill(spk, 32, rnd=False)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    D = {k: T(v) for k, v in dict(e_sig=e_sig, e_msg=e_msg, e_pk=e_pk, r_sig=r_sig, r_msg=r_msg, r_id=r_id, s_sig=s_sig, s_msg=s_msg, s_pk=s_pk).items()}
    res = torch.zeros(nmax, dtype=torch.int32, device=dev); keys = torch.zeros((nmax, 64), dtype=torch.uint8, device=dev)
    eng = Engine(0)
    diag = bool(os.environ.get("S2K_LIB"))
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "diagnostic_library": diag, "device": torch.cuda.get_device_name(0), "reps": a.reps, "reference_made_items": NV, "sizes": {}}
    for n in a.sizes:
        row = {}
        ms = timed(eng, lambda: eng.ecdsa_verify_batch_dev(res[:n], D["e_sig"][:n], D["e_msg"][:n], D["e_pk"][:n], n=n), a.reps)
        got = res[:n].cpu().numpy()
        if not diag:
            assert got[:NV].all() and not got[NV:].any(), "k_ecdsa_verify: wrong verdicts"
        row["ecdsa_verify"] = stats(ms, n)
        ms = timed(eng, lambda: eng.ecdsa_recover_batch_dev(res[:n], keys[:n], D["r_sig"][:n], D["r_id"][:n], D["r_msg"][:n], n=n), a.reps)
        if not diag:
            assert res[:n].cpu().numpy().all() and np.array_equal(keys[:min(n, NV)].cpu().numpy(), rpk[:n]), "k_ecdsa_recover: wrong results"
        row["ecdsa_recover"] = stats(ms, n)
        ms = timed(eng, lambda: eng.schnorrsig_verify_batch_dev(res[:n], D["s_sig"][:n], D["s_msg"][:n], D["s_pk"][:n]), a.reps)
        got = res[:n].cpu().numpy()
        assert got[:NV].all() and not got[NV:].any(), "k_schnorr_verify: wrong verdicts"
        row["bip340_verify"] = stats(ms, n)
        row["ecdsa_verify_over_bip340"] = round(row["ecdsa_verify"]["items_per_s"] / row["bip340_verify"]["items_per_s"], 4)
        row["ecdsa_recover_over_bip340"] = round(row["ecdsa_recover"]["items_per_s"] / row["bip340_verify"]["items_per_s"], 4)
        out["sizes"][str(n)] = row
    if not a.no_cpu:
        out["reference_cpu_ecdsa_verify"] = ref_cpu_figure()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
