#!/usr/bin/env python3
"""Diagnostic: the share of the per-lane scalar inversion (sc_inverse: variable-time division steps, the lanes of a wavefront diverge) in
k_ecdsa_verify and k_ecdsa_recover, as the difference between the product library and a build that replaces the inversion by a copy
(-DS2K_ECDSA_DIAG_NO_SCINV, csrc/ecdsa.h; verdicts are meaningless in that build).  Build the variant first, then on the GPU box:
    python -m secp256k1_zkp_amd.build_lib -o /tmp/libs2k_ecdsa_noscinv.so -DS2K_ECDSA_DIAG_NO_SCINV
    python tools/ecdsa_parts.py /tmp/libs2k_ecdsa_noscinv.so [--into rates.json] [n ...]
--into: add the result as the "scalar_inversion_share" block of a file tools/ecdsa_bare.py --out wrote (profiles/ecdsa_rates.json is made so);
refused when that file was measured with another library than the product runs here.
Each library is timed in a fresh child process (tools/ecdsa_bare.py), product, variant, product again: the two product runs bound the
run-to-run noise the difference has to be read against."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(lib, sizes):
    env = dict(os.environ)
    env.pop("S2K_LIB", None)
    if lib:
        env["S2K_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ecdsa_bare.py"), "--no-cpu", "--sizes"] + [str(s) for s in sizes], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit(p.returncode)
    return json.loads(p.stdout)


def main():
    args = sys.argv[1:]
    into = None
    if "--into" in args:
        i = args.index("--into"); into = args[i + 1]; del args[i:i + 2]
    lib = os.path.abspath(args[0])
    sizes = [int(x) for x in args[1:]] or [1 << 16, 1 << 20]
    a, v, b = run(None, sizes), run(lib, sizes), run(None, sizes)
    out = {"so_sha256": a["so_sha256"], "variant_so_sha256": v["so_sha256"], "git_head": a["git_head"], "sizes": {}}
    for n in map(str, sizes):
        row = {}
        for k in ("ecdsa_verify", "ecdsa_recover"):
            p1, p2, nv = a["sizes"][n][k]["ms_median"], b["sizes"][n][k]["ms_median"], v["sizes"][n][k]["ms_median"]
            p = 0.5 * (p1 + p2)
            row[k] = {"product_ms": [p1, p2], "no_scalar_inversion_ms": nv, "scalar_inversion_share_pct": round(100 * (p - nv) / p, 2),
                      "product_run_to_run_pct": round(100 * abs(p1 - p2) / p, 2)}
        out["sizes"][n] = row
    print(json.dumps(out, indent=1))
    if into:
        rates = json.load(open(into))
        if rates.get("so_sha256") != out["so_sha256"]:
            raise SystemExit("%s was measured with another library (so_sha256 differs)" % into)
        rates["scalar_inversion_share"] = {"tool": "tools/ecdsa_parts.py", "variant": "-DS2K_ECDSA_DIAG_NO_SCINV", "variant_so_sha256": out["variant_so_sha256"], "sizes": out["sizes"]}
        with open(into, "w") as f:
            f.write(json.dumps(rates, indent=1) + "\n")


if __name__ == "__main__":
    main()
