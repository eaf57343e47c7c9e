#!/usr/bin/env python3
"""Device-resident timing of k_musig_partial_verify and k_musig_nonce_process (secp256k1_musig_partial_sig_verify_batch_dev,
secp256k1_musig_nonce_process_batch_dev) next to k_ecdsa_verify (secp256k1_ecdsa_verify_batch_dev) in the same process, on the same box,
at the same n:

    python tools/musig_bare.py [--sizes 65536 1048576] [--rounds 3] [--out profiles/musig_rates.json]
    python tools/musig_bare.py --ab two_call.so [--ab-rounds 3] ...     (two_call.so: python -m secp256k1_zkp_amd.build_lib -o two_call.so -DS2K_MUSIG_JOINT=0)

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)).  After two warm-up calls of each, the kernels
alternate for --rounds rounds; every figure is the median of the rounds with their minimum and maximum (the spread) beside it.  The
verifier runs in the object formats (no square root) and in the serialised ones (two lifts for the pubnonce, one for a compressed key),
the processor likewise, with and without adaptors.  --ab runs 2^17 items again in child processes that alternate between the default
library (joint form) and the given one (two-call form), in the way of tools/ab_probe.py, and records both rates and their ranges.

Inputs.  Every share is valid under the verification equation  s*G = e'*P + sigma*(R1 + b*R2): the points (P = x G, R1 = k1 G, R2 = k2 G)
come from the engine's own s2k_ecmult_batch, the key coefficients from hashlib and s from Python integers.  64 sessions (b, e and the
nonce parity drawn at random) and 64 caches (an aggregate key, a second key that is no signer's, a key-list hash) are shared through
session_of, as a coordinator shares them among the signers of a session; the verifier reads nothing else of them.  One share in 256
has a bit flipped: it runs every stage and fails the comparison.  The processor gets the shares' nonces as aggregate nonces, fresh
messages, the caches expanded to one per item and one adaptor point per item; all its verdicts are 1, and the nonce coefficients of 64
sessions it wrote are compared with hashlib.  The ECDSA items are made from the same keys and nonces.  All verdicts are checked."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from secp256k1_zkp_amd import Engine, _native  # noqa: E402
from secp256k1_zkp_amd.constants import N, G_XY  # noqa: E402

N_SESSIONS = 64
MAGIC = dict(cache=bytes([0xf4, 0xad, 0xbb, 0xdf]), pubnonce=bytes([0xf5, 0x7a, 0x3d, 0xa0]), aggnonce=bytes([0xa8, 0xb7, 0xe4, 0x67]),
             session=bytes([0x9d, 0xed, 0xe9, 0x17]), sig=bytes([0xeb, 0xfb, 0x1a, 0x32]))


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


def make_items(eng, n, rng):
    """-> dict of uint8 arrays (both representations of shares, nonces and keys; caches, sessions, session_of; the processor's and the
    ECDSA kernel's inputs) and the expected verify verdicts"""
    def scalars(k):
        a = rng.integers(0, 256, (k, 32), dtype=np.uint8); a[:, 0] &= 0x7F; a[:, 31] |= 1      # in [1, 2^255): below n, nonzero
        return a
    ints = lambda a: [int.from_bytes(r.tobytes(), "big") for r in a]      # noqa: E731
    gmul = lambda s: eng.ecmult_batch(np.tile(np.frombuffer(G_XY, np.uint8), (len(s), 1)), np.zeros((len(s), 32), np.uint8), ng=s)[0]      # noqa: E731
    ser = lambda P: np.concatenate([(2 + (P[:, 63] & 1))[:, None], P[:, :32]], axis=1).astype(np.uint8)      # noqa: E731
    obj = lambda P: np.concatenate([P[:, 31::-1], P[:, :31:-1]], axis=1)      # x, y as 32 little-endian bytes each      # noqa: E731
    x, k1, k2 = scalars(n), scalars(n), scalars(n)
    X, R1, R2 = gmul(x), gmul(k1), gmul(k2)
    sX = ser(X)
    # the pairs
    Q, second = gmul(scalars(N_SESSIONS)), gmul(scalars(N_SESSIONS))
    pks_hash = rng.integers(0, 256, (N_SESSIONS, 32), dtype=np.uint8)
    b, e = scalars(N_SESSIONS), scalars(N_SESSIONS)
    parity = rng.integers(0, 2, N_SESSIONS, dtype=np.uint8)
    caches = np.zeros((N_SESSIONS, 197), np.uint8); sessions = np.zeros((N_SESSIONS, 133), np.uint8)
    caches[:, :4] = np.frombuffer(MAGIC["cache"], np.uint8); caches[:, 4:68] = obj(Q); caches[:, 68:132] = obj(second); caches[:, 132:164] = pks_hash
    sessions[:, :4] = np.frombuffer(MAGIC["session"], np.uint8); sessions[:, 4] = parity; sessions[:, 37:69] = b; sessions[:, 69:101] = e
    of = (np.arange(n) % N_SESSIONS).astype(np.uint32)
    bi, ei, q_odd = ints(b), ints(e), (Q[:, 63] & 1)
    xi, k1i, k2i = ints(x), ints(k1), ints(k2)
    sig = np.zeros((n, 32), np.uint8); esig = np.zeros((n, 64), np.uint8)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kinv = pow_batch(k1i)
    for i in range(n):
        S = i % N_SESSIONS
        mu = int.from_bytes(tagged(b"KeyAgg coefficient", pks_hash[S].tobytes() + sX[i].tobytes()), "big") % N
        e1 = ei[S] * mu % N
        if q_odd[S]:                                                       # parity_acc is 0: e' is negated iff y(Q) is odd
            e1 = N - e1
        nonce = (k1i[i] + bi[S] * k2i[i]) % N
        s = (e1 * xi[i] + (N - nonce if parity[S] else nonce)) % N
        sig[i] = np.frombuffer(s.to_bytes(32, "big"), np.uint8)
        r2 = int.from_bytes(R1[i, :32].tobytes(), "big") % N               # ECDSA under the same key with the nonce k1
        m = int.from_bytes(msg[i].tobytes(), "big") % N
        s2 = (m + r2 * xi[i]) * kinv[i] % N
        s2 = min(s2, N - s2)
        assert r2 and s2
        esig[i] = np.frombuffer(r2.to_bytes(32, "big") + s2.to_bytes(32, "big"), np.uint8)
    exp = np.ones(n, np.int32)
    bad = np.arange(255, n, 256)
    sig[bad, 31] ^= 1; exp[bad] = 0
    D = dict(sig0=sig, sig1=np.concatenate([np.tile(np.frombuffer(MAGIC["sig"], np.uint8), (n, 1)), sig], axis=1),
             nonce0=np.concatenate([ser(R1), ser(R2)], axis=1), nonce1=np.concatenate([np.tile(np.frombuffer(MAGIC["pubnonce"], np.uint8), (n, 1)), obj(R1), obj(R2)], axis=1),
             pk0=sX, pk1=obj(X), caches=caches, sessions=sessions, of=of.view(np.int32),
             agg0=np.concatenate([ser(R1), ser(R2)], axis=1), agg1=np.concatenate([np.tile(np.frombuffer(MAGIC["aggnonce"], np.uint8), (n, 1)), obj(R1), obj(R2)], axis=1),
             msg=msg, pcaches=caches[of], adaptor=obj(X), esig=esig)
    return D, exp


def pow_batch(vals):
    """1/v mod n for every v (none zero) with one modular inversion"""
    pre, run = [], 1
    for v in vals:
        pre.append(run); run = run * v % N
    inv = pow(run, -1, N)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % N; inv = inv * vals[i] % N
    return out


def measure(eng, D, exp, n, rounds, only_verify=False):
    dev = torch.device("cuda", 0)
    per_item = ("caches", "sessions")
    d = {k: torch.from_numpy(np.ascontiguousarray(v if k in per_item else v[:n])).to(dev) for k, v in D.items()}
    res = torch.zeros(n, dtype=torch.int32, device=dev); out = torch.zeros((n, 133), dtype=torch.uint8, device=dev)
    ver = lambda f: eng.musig_partial_sig_verify_dev(res, d["sig%d" % f], d["nonce%d" % f], d["pk%d" % f], d["caches"], d["sessions"], N_SESSIONS, session_of=d["of"],      # noqa: E731
                                                     sig_format=f, nonce_format=f, pk_format=f, n=n)
    pro = lambda f, ad: eng.musig_nonce_process_dev(res, out, d["agg%d" % f], d["msg"], d["pcaches"], adaptors=d["adaptor"] if ad else None, nonce_format=f, n=n)      # noqa: E731
    ec = lambda: eng.ecdsa_verify_batch_dev(res, d["esig"], d["msg"], d["pk0"], n=n)      # noqa: E731
    calls = {"verify_objects": lambda: ver(1), "verify_serialised": lambda: ver(0)}
    if not only_verify:
        calls.update({"process_objects": lambda: pro(1, False), "process_serialised": lambda: pro(0, False), "process_objects_adaptor": lambda: pro(1, True),
                      "ecdsa_verify": ec})
    for _ in range(2):
        for name, call in calls.items():
            call(); eng.sync()
            got = res.cpu().numpy()
            assert np.array_equal(got, exp[:n]) if name.startswith("verify") else got.all(), name + ": wrong verdicts"
            if name == "process_objects":
                sess = out[:64].cpu().numpy()
                for i in range(min(n, 64)):
                    want = tagged(b"MuSig/noncecoef", D["agg0"][i].tobytes() + D["pcaches"][i, 35:3:-1].tobytes() + D["msg"][i].tobytes())
                    assert int.from_bytes(sess[i, 37:69].tobytes(), "big") == int.from_bytes(want, "big") % N, "k_musig_nonce_process: wrong nonce coefficient"
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            call(); eng.sync(); ms[name].append(eng.last_ms(1))
    row = {k: stats(v, n) for k, v in ms.items()}
    if not only_verify:
        ecd = row["ecdsa_verify"]["ms_median"]
        row["item_time_over_ecdsa_item_time"] = {k: round(v["ms_median"] / ecd, 3) for k, v in row.items() if k != "ecdsa_verify"}
        row["serialised_over_objects"] = {"verify": round(row["verify_serialised"]["ms_median"] / row["verify_objects"]["ms_median"], 3),
                                          "process": round(row["process_serialised"]["ms_median"] / row["process_objects"]["ms_median"], 3)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", default=None, help="a library built with -DS2K_MUSIG_JOINT=0 to alternate with")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-size", type=int, default=1 << 17, help="items per call in the A/B children (each child makes its own inputs)")
    ap.add_argument("--reference-us", type=float, nargs=2, default=None, metavar=("VERIFY", "PROCESS"),
                    help="the reference's time per call on one core, as tests/golden/make_musig_golden.py --time printed it: recorded as given")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    rng = np.random.default_rng(43)
    eng = Engine(0)
    D, exp = make_items(eng, max(a.sizes), rng)
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    out = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "corrupted_one_in": 256, "sessions_shared": N_SESSIONS, "sizes": {}}
    for n in a.sizes:
        out["sizes"][str(n)] = measure(eng, D, exp, n, a.rounds, only_verify=a.child)
    eng.close()
    if a.child:
        print("RESULT " + json.dumps(out["sizes"][str(max(a.sizes))]["verify_objects"]))
        return
    if a.ab:
        n = a.ab_size
        libs = {"joint (default library)": _native.LIB_PATH, "two-call (-DS2K_MUSIG_JOINT=0)": os.path.abspath(a.ab)}
        runs = {k: [] for k in libs}
        for _ in range(a.ab_rounds):
            for name, lib in libs.items():
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", str(n), "--rounds", str(a.rounds)], env=dict(os.environ, S2K_LIB=lib),
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if not line:
                    raise SystemExit("child failed (%s): %s" % (name, p.stderr[-800:]))
                runs[name].append(json.loads(line[0][7:]))
        ab = {"n": n, "kernel": "k_musig_partial_verify, object formats", "runs": runs}
        med = {k: sorted(r["ms_median"] for r in v)[len(v) // 2] for k, v in runs.items()}
        rng_ms = {k: [min(r["ms_min"] for r in v), max(r["ms_max"] for r in v)] for k, v in runs.items()}
        j, t = "joint (default library)", "two-call (-DS2K_MUSIG_JOINT=0)"
        ab["ms_median"] = med; ab["ms_range"] = rng_ms
        ab["us_per_item"] = {k: round(1e3 * v / n, 5) for k, v in med.items()}
        ab["joint_faster_by_pct"] = round(100 * (med[t] - med[j]) / med[t], 2)
        ab["ranges_clear"] = bool(rng_ms[j][1] < rng_ms[t][0])
        ab["joint_stays_default"] = bool(med[j] < med[t] and rng_ms[j][1] < rng_ms[t][0])
        out["joint_vs_two_call"] = ab
    if a.reference_us:
        out["reference_cpu_us_per_call"] = {"secp256k1_musig_partial_sig_verify": a.reference_us[0], "secp256k1_musig_nonce_process": a.reference_us[1],
                                            "source": "tests/golden/make_musig_golden.py --time, one core of the build machine, ctypes call overhead included"}
    else:
        out["reference_cpu_us_per_call"] = "not measured here: the reference's module is only compiled by tests/golden/make_musig_golden.py --time, which needs the reference's sources"
    text = compact(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
