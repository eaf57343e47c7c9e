#!/usr/bin/env python3
"""Device-resident timing of the generator and commitment kernels through their `_dev` entry points -- parse, serialize, generate,
generate blinded, commit with NULL blinds, commit with blinds -- alternating in the same process, on the same box, at the same n, with
s2k_ecmult_batch_dev on random scalars beside them (a general double multiplication: what the commit kernel is built on).

    python tools/generator_bare.py [--sizes 65536 1048576] [--reps 7] [--out profiles/generator_rates.json]

Times are the HIP events the engine records around its launches (s2k_engine_last_ms(1)), after two warm-up calls of every routine; every
figure is the median of --reps calls with their minimum and maximum beside it.  One round of the measured loop calls every routine once, so
that a drift of the box lands on all of them alike.  The run is APPENDED to --out (a JSON list of runs), stamped with the commit
($S2K_GIT_HEAD) and the library's hash.

Gate: at 2^20 items the generate rate must be at least 1/8 of the parse rate of the same run (six square-root chains against one, two
wave-shared inversions, about forty products and two hash blocks; per-lane inversions would add roughly two chains and miss it).

Inputs (oracle/_ref must be built: every expected value is the reference's).  Random asset ids, distinct random blinds below n, random
64-bit values.  The generator objects the other kernels read are the generate kernel's own output, whose first 2^12 items are compared
with the reference byte for byte, as are the first 2^12 outputs of every other routine."""
import argparse
import ctypes
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

NV = 1 << 12


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


def ref_cpu_figures(gref, keys, blinds, values, gens64, gens33, iters=2000):
    """the reference's functions in a loop on one core of this box, through tests/generator_ref.py (the ctypes call overhead, about a
    microsecond, is inside every figure)"""
    L, ctx = gref.lib, gref.ctx
    m = min(iters, len(keys))
    K = [keys[i].tobytes() for i in range(m)]; B = [blinds[i].tobytes() for i in range(m)]; V = [int(values[i]) for i in range(m)]
    G = [gens64[i].tobytes() for i in range(m)]; S = [gens33[i].tobytes() for i in range(m)]
    o = ctypes.create_string_buffer(64)
    out = {}

    def loop(name, f):
        ok = 0
        t0 = time.perf_counter()
        for i in range(m):
            ok += f(i)
        dt = time.perf_counter() - t0
        assert ok == m, name
        out[name] = {"calls": m, "us_per_call": round(dt / m * 1e6, 3), "per_s_one_core": round(m / dt, 1)}
    loop("secp256k1_generator_parse", lambda i: L.secp256k1_generator_parse(ctx, o, S[i]))
    loop("secp256k1_generator_serialize", lambda i: L.secp256k1_generator_serialize(ctx, o, G[i]))
    loop("secp256k1_generator_generate", lambda i: L.secp256k1_generator_generate(ctx, o, K[i]))
    loop("secp256k1_generator_generate_blinded", lambda i: L.secp256k1_generator_generate_blinded(ctx, o, K[i], B[i]))
    loop("secp256k1_pedersen_commit", lambda i: L.secp256k1_pedersen_commit(ctx, o, B[i], V[i], G[i]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generator_rates.json"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if min(a.sizes) < 1:
        ap.error("--sizes: every size must be at least 1")
    if not os.path.exists(REF_PATH):                  # every expected output is the reference's: nothing is timed unchecked
        raise SystemExit("tools/generator_bare.py: oracle/_ref is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tests.generator_ref import GeneratorRef
    gref = GeneratorRef()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(43)
    nmax = max(max(a.sizes), NV)
    keys = rng.integers(0, 256, (nmax, 32), dtype=np.uint8)
    blinds = rng.integers(0, 256, (nmax, 32), dtype=np.uint8); blinds[:, 0] &= 0x7F          # distinct, below n
    scal = rng.integers(0, 256, (nmax, 32), dtype=np.uint8); scal[:, 0] &= 0x7F
    values = rng.integers(1, 1 << 64, nmax, dtype=np.uint64)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    D = {"keys": T(keys), "blinds": T(blinds), "scal": T(scal), "values": T(values.view(np.int64))}
    z64 = lambda: torch.zeros((nmax, 64), dtype=torch.uint8, device=dev)      # noqa: E731
    z33 = lambda: torch.zeros((nmax, 33), dtype=torch.uint8, device=dev)      # noqa: E731
    zr = lambda: torch.zeros(nmax, dtype=torch.int32, device=dev)             # noqa: E731
    res = {k: zr() for k in ("parse", "generate", "generate_blinded", "commit_null", "commit_blinds")}
    out = {"parse": z64(), "serialize": z33(), "generate": z64(), "generate_blinded": z64(), "commit_null": z33(), "commit_blinds": z33()}
    r_xy = z64(); r_inf = zr()
    eng = Engine(0)
    # the inputs of the other kernels: generator objects and their serialisations, made once by the engine and checked below
    gens64 = z64(); gens33 = z33(); r0 = zr()
    eng.generator_generate_batch_dev(r0, gens64, D["keys"], None, n=nmax)
    eng.generator_serialize_batch_dev(gens33, gens64, n=nmax)
    eng.sync()
    assert r0.cpu().numpy().all()
    h_gens64 = gens64.cpu().numpy(); h_gens33 = gens33.cpu().numpy()
    want = {"parse": [], "serialize": [], "generate": [], "generate_blinded": [], "commit_null": [], "commit_blinds": []}
    for i in range(NV):
        g = gref.generate(keys[i].tobytes()); assert g[0] == 1
        want["generate"].append(g[1]); want["serialize"].append(gref.serialize(g[1])); want["parse"].append(g[1])
        gb = gref.generate(keys[i].tobytes(), blinds[i].tobytes()); assert gb[0] == 1
        want["generate_blinded"].append(gb[1])
        c = gref.commit(None, int(values[i]), g[1]); assert c[0] == 1
        want["commit_null"].append(c[1])
        c = gref.commit(blinds[i].tobytes(), int(values[i]), g[1]); assert c[0] == 1
        want["commit_blinds"].append(c[1])
    want = {k: np.frombuffer(b"".join(v), np.uint8).reshape(NV, -1) for k, v in want.items()}
    assert np.array_equal(h_gens64[:NV], want["generate"]) and np.array_equal(h_gens33[:NV], want["serialize"]), "input generators differ from the reference's"
    so_sha = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()
    run = {"so_sha256": so_sha, "src_sha256": _native.sources_sha256(), "git_head": os.environ.get("S2K_GIT_HEAD", "unknown"), "library": os.path.basename(_native.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "reference_checked_items": NV, "sizes": {}}
    for n in a.sizes:
        calls = {
            "parse": lambda: eng.generator_parse_batch_dev(res["parse"][:n], out["parse"][:n], gens33[:n], n=n),
            "generate": lambda: eng.generator_generate_batch_dev(res["generate"][:n], out["generate"][:n], D["keys"][:n], None, n=n),
            "serialize": lambda: eng.generator_serialize_batch_dev(out["serialize"][:n], gens64[:n], n=n),
            "generate_blinded": lambda: eng.generator_generate_batch_dev(res["generate_blinded"][:n], out["generate_blinded"][:n], D["keys"][:n], D["blinds"][:n], n=n),
            "commit_null": lambda: eng.pedersen_commit_batch_dev(res["commit_null"][:n], out["commit_null"][:n], D["values"][:n], gens64[:n], None, n=n),
            "commit_blinds": lambda: eng.pedersen_commit_batch_dev(res["commit_blinds"][:n], out["commit_blinds"][:n], D["values"][:n], gens64[:n], D["blinds"][:n], n=n),
            "ecmult_batch_random_scalars": lambda: eng.ecmult_batch_dev(r_xy[:n], r_inf[:n], gens64[:n], D["scal"][:n], ng=D["blinds"][:n]),
        }
        ms = timed_alternating(eng, calls, a.reps)
        m = min(n, NV)
        for k in out:
            if k in res:
                assert res[k][:n].cpu().numpy().all(), "%s: a result is 0" % k
            assert np.array_equal(out[k][:m].cpu().numpy(), want[k][:m]), "%s: output differs from the reference's" % k
        assert not r_inf[:n].cpu().numpy().any()
        row = {k: stats(v, n) for k, v in ms.items()}
        row["generate_over_parse"] = round(row["generate"]["items_per_s"] / row["parse"]["items_per_s"], 4)
        row["commit_blinds_over_ecmult_batch"] = round(row["commit_blinds"]["items_per_s"] / row["ecmult_batch_random_scalars"]["items_per_s"], 4)
        run["sizes"][str(n)] = row
    top = run["sizes"].get(str(1 << 20))
    if top:
        run["gate_generate_at_least_one_eighth_of_parse_at_2^20"] = bool(top["generate"]["items_per_s"] * 8 >= top["parse"]["items_per_s"])
    if not a.no_cpu:
        run["reference_cpu"] = ref_cpu_figures(gref, keys, blinds, values, h_gens64, h_gens33)
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
