#!/usr/bin/env python3
"""Device-resident timing of k_tweak_check and k_tweak_add through the `_dev` entry points at key_format 0 and 1, alternating in the same
process, on the same box, at the same n, with what a caller had before them: s2k_ecmult_batch_dev with na = 1, ng = t on the same keys
(the comparator: a general double multiplication, no key parsing, no comparison, no verdict).  k_schnorr_verify is timed as a second
line, for orientation.

    python tools/tweak_bare.py [--sizes 65536 1048576] [--reps 7] [--out profiles/tweak_rates.json]

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)), after two warm-up calls of every routine; every
figure is the median of --reps calls with their minimum and maximum beside it.  One round of the measured loop calls every routine once, so
that a drift of the box lands on all of them alike.  The run is APPENDED to --out (a JSON list of runs), stamped with the commit
($S2K_GIT_HEAD) and the library's hash.

Inputs (oracle/_ref must be built: the keys and every expected value are the reference's).  Valid keys (1 024 of them, tiled) under
DISTINCT random tweaks, so that no generator-table address repeats.  The first 2^14 items carry the reference's output key and parity
and are checked: check verdict 1, add output equal byte for byte, comparator point equal.  The rest carry random tweaked32 bytes: they run the whole item and are refused by the final
comparison only (checked: verdict 0; the add form accepts them)."""
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
from tests.refapi import REF_PATH  # noqa: E402

NV = 1 << 14
NKEYS = 1 << 10


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "spread_pct": round(100 * (ms[-1] - ms[0]) / med, 2),
            "items_per_s": round(n / med * 1e3, 1)}


def timed_alternating(eng, calls, reps):
    """calls: {name: callable} -> {name: [ms] * reps}; two warm-up rounds, then reps rounds of every call once"""
    for _ in range(2):
        for c in calls.values():
            c(); eng.sync()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            c(); eng.sync()
            ms[k].append(eng.last_ms(1))
    return ms


def ref_cpu_figure(tref, keys_obj, tweaks, tweaked, par, iters=20000):
    """secp256k1_xonly_pubkey_tweak_add_check of the reference in a loop on one core of this box, through tests/tweak_ref.py (the ctypes
    call overhead, about a microsecond, is inside the figure)"""
    f = tref.lib.secp256k1_xonly_pubkey_tweak_add_check; ctx = tref.ctx
    args = [(tweaked[i].tobytes(), int(par[i]), keys_obj[i].tobytes(), tweaks[i].tobytes()) for i in range(min(iters, len(par)))]
    ok = 0
    t0 = time.perf_counter()
    for tw, p, k, t in args:
        ok += f(ctx, tw, p, k, t)
    dt = time.perf_counter() - t0
    assert ok == len(args)
    return {"calls": len(args), "us_per_call": round(dt / len(args) * 1e6, 3), "checks_per_s_one_core": round(len(args) / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tweak_rates.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(41)
    have_ref = os.path.exists(REF_PATH)
    nmax = max(max(a.sizes), NV)
    tweaks = rng.integers(0, 256, (nmax, 32), dtype=np.uint8); tweaks[:, 0] &= 0x7F          # distinct, below n
    tweaked = rng.integers(0, 256, (nmax, 32), dtype=np.uint8); par = rng.integers(0, 2, nmax, dtype=np.uint8)
    if not have_ref:                         # the keys and the expected outputs are the reference's: nothing is timed unchecked
        raise SystemExit("tools/tweak_bare.py: oracle/_ref is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tests.tweak_ref import TweakRef, obj_x32, obj_parity
    tref = TweakRef()
    kobj = [tref.xonly_from_pubkey(tref.ec_create(bytes(rng.integers(0, 256, 31, dtype=np.uint8).tolist()) + b"\x01"))[0] for _ in range(NKEYS)]
    keys_obj = np.frombuffer(b"".join(kobj), np.uint8).reshape(NKEYS, 64)
    want_out = np.zeros((NV, 64), np.uint8)
    for i in range(NV):
        v, o = tref.add(1, kobj[i % NKEYS], tweaks[i].tobytes())
        assert v
        want_out[i] = np.frombuffer(o, np.uint8); tweaked[i] = np.frombuffer(obj_x32(o), np.uint8); par[i] = obj_parity(o)
    reps_of = (nmax + NKEYS - 1) // NKEYS
    keys_obj_all = np.tile(keys_obj, (reps_of, 1))[:nmax]
    keys_x = np.ascontiguousarray(keys_obj_all[:, 31::-1])                                    # serialised x-only keys (even y: the objects are x-only objects)
    a_xy = np.concatenate([keys_x, keys_obj_all[:, :31:-1]], axis=1)                          # x | y big-endian for s2k_ecmult_batch
    one = np.zeros((nmax, 32), np.uint8); one[:, 31] = 1
    # BIP-340, for orientation: reference-made signatures in front, random r / s below 2^255 behind them, valid keys tiled
    from tests.refapi import Ref
    ssig, smsg, spk = Ref().make_schnorr(NV, rng, threads=16)
    s_sig = rng.integers(0, 256, (nmax, 64), dtype=np.uint8); s_sig[:, 0] &= 0x7F; s_sig[:, 32] &= 0x7F; s_sig[:NV] = ssig
    s_msg = rng.integers(0, 256, (nmax, 32), dtype=np.uint8); s_msg[:NV] = smsg
    s_pk = np.tile(spk, ((nmax + NV - 1) // NV, 1))[:nmax]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    D = {k: T(v) for k, v in dict(tweaks=tweaks, tweaked=tweaked, par=par, kobj=keys_obj_all, kx=keys_x, a_xy=a_xy, one=one, s_sig=s_sig, s_msg=s_msg, s_pk=s_pk).items()}
    res = {k: torch.zeros(nmax, dtype=torch.int32, device=dev) for k in ("c0", "c1", "a0", "a1", "s")}
    outk = {k: torch.zeros((nmax, 64), dtype=torch.uint8, device=dev) for k in ("a0", "a1")}
    r_xy = torch.zeros((nmax, 64), dtype=torch.uint8, device=dev); r_inf = torch.zeros(nmax, dtype=torch.int32, device=dev)
    eng = Engine(0)
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    run = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "reference_checked_items": NV, "sizes": {}}
    for n in a.sizes:
        calls = {
            "tweak_check_fmt1": lambda: eng.xonly_tweak_add_check_batch_dev(res["c1"][:n], D["tweaked"][:n], D["par"][:n], D["kobj"][:n], D["tweaks"][:n], key_format=1, n=n),
            "tweak_add_fmt1": lambda: eng.pubkey_tweak_add_batch_dev(res["a1"][:n], outk["a1"][:n], D["kobj"][:n], D["tweaks"][:n], key_format=1, n=n),
            "comparator_ecmult_batch_na1": lambda: eng.ecmult_batch_dev(r_xy[:n], r_inf[:n], D["a_xy"][:n], D["one"][:n], ng=D["tweaks"][:n]),
            "tweak_check_fmt0": lambda: eng.xonly_tweak_add_check_batch_dev(res["c0"][:n], D["tweaked"][:n], D["par"][:n], D["kx"][:n], D["tweaks"][:n], key_format=0, n=n),
            "tweak_add_fmt0": lambda: eng.pubkey_tweak_add_batch_dev(res["a0"][:n], outk["a0"][:n], D["kx"][:n], D["tweaks"][:n], key_format=0, n=n),
            "bip340_verify": lambda: eng.schnorrsig_verify_batch_dev(res["s"][:n], D["s_sig"][:n], D["s_msg"][:n], D["s_pk"][:n]),
        }
        ms = timed_alternating(eng, calls, a.reps)
        m = min(n, NV)
        for k in ("c0", "c1"):
            got = res[k][:n].cpu().numpy()
            assert got[:m].all() and not got[NV:].any(), "k_tweak_check: wrong verdicts (%s)" % k
        for k in ("a0", "a1"):
            assert res[k][:n].cpu().numpy().all() and np.array_equal(outk[k][:m].cpu().numpy(), want_out[:m]), "k_tweak_add: wrong results (%s)" % k
        cmp_xy = r_xy[:m].cpu().numpy()
        assert not r_inf[:n].cpu().numpy().any() and np.array_equal(cmp_xy[:, :32], want_out[:m, 31::-1]) and np.array_equal(cmp_xy[:, 32:], want_out[:m, :31:-1]), "comparator: wrong points"
        assert np.array_equal(outk["a1"][:n].cpu().numpy()[:, 31::-1], r_xy[:n].cpu().numpy()[:, :32]), "add form and comparator disagree"
        got = res["s"][:n].cpu().numpy()
        assert got[:m].all() and not got[NV:].any(), "k_schnorr_verify: wrong verdicts"
        row = {k: stats(v, n) for k, v in ms.items()}
        c = row["comparator_ecmult_batch_na1"]
        for k in ("tweak_check_fmt1", "tweak_add_fmt1", "tweak_check_fmt0", "tweak_add_fmt0"):
            row[k]["over_comparator"] = round(row[k]["items_per_s"] / c["items_per_s"], 3)
            row[k]["range_clear_of_comparator"] = bool(row[k]["ms_max"] < c["ms_min"])
        row["lift_share_of_check_fmt0"] = round(1 - row["tweak_check_fmt1"]["ms_median"] / row["tweak_check_fmt0"]["ms_median"], 4)
        row["lift_share_of_add_fmt0"] = round(1 - row["tweak_add_fmt1"]["ms_median"] / row["tweak_add_fmt0"]["ms_median"], 4)
        run["sizes"][str(n)] = row
    top = run["sizes"].get(str(1 << 20))
    if top:
        run["gate_faster_than_comparator_at_2^20_fmt1"] = bool(top["tweak_check_fmt1"]["range_clear_of_comparator"] and top["tweak_add_fmt1"]["range_clear_of_comparator"])
        run["mark_3x_comparator_at_2^20_fmt1"] = {"check": "hit" if top["tweak_check_fmt1"]["over_comparator"] >= 3 else "missed",
                                                  "add": "hit" if top["tweak_add_fmt1"]["over_comparator"] >= 3 else "missed"}
    if not a.no_cpu:
        run["reference_cpu_xonly_tweak_add_check"] = ref_cpu_figure(tref, keys_obj_all[:NV], tweaks[:NV], tweaked[:NV], par[:NV])
    run["gtab_bits"] = int(eng._lib.s2k_engine_gtable_bits(eng._h))
    eng.close()
    print(json.dumps(run, indent=1))
    runs = []
    if os.path.exists(a.out):
        with open(a.out) as f:
            runs = json.load(f)
    runs.append(run)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(runs, indent=1) + "\n")


if __name__ == "__main__":
    main()
