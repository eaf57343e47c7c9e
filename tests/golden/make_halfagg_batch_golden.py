#!/usr/bin/env python3
"""Writes tests/golden/halfagg_batch_vectors.json: half-aggregates of 0, 1, 2, 3, 4, 5, 16 and 40 BIP-340 signatures as the reference's
secp256k1_schnorrsig_aggregate made them, tampered copies of each with the verdict the reference's secp256k1_schnorrsig_aggverify
returned when the file was written, and one (key, message, signature) triple with the reference's final s for that triple repeated
4 097 times (the aggregate above the many-sums limit; expanded at test time).

Run once in the build container, after build() has made oracle/_ref:   python tests/golden/make_halfagg_batch_golden.py
Uses tests/refapi.py (halfagg_aggregate, halfagg_verify, the shim's signing helper make_schnorr, xonly_objects).  No test runs it.

A tampered copy is recorded as patches to its base: [field, byte offset, hex] overwrites bytes of "pks" / "msgs" / "agg"; "agg_len"
truncates or zero-extends the aggregate.  A patch of "pks" is applied to the 32-byte keys; the 64-byte key objects ("objs", as
secp256k1_xonly_pubkey holds them) of the patched keys are recorded with it: the reference's own for keys that parse, 64 zero bytes
(the object the engine documents as refused) for one that does not."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.refapi import Ref, P, N      # noqa: E402

SIZES = (0, 1, 2, 3, 4, 5, 16, 40)
BIG = 4097


def not_an_x(rng):
    """32 bytes below p that are not the x coordinate of a curve point"""
    while True:
        x = int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % P
        if pow((x * x * x + 7) % P, (P - 1) // 2, P) != 1:
            return x.to_bytes(32, "big")


def apply(base, patches):
    pks, msgs, agg = bytearray(base["pks"]), bytearray(base["msgs"]), bytearray(base["agg"])
    for f, off, hx in patches:
        b = bytes.fromhex(hx) if isinstance(hx, str) else hx
        if f == "agg_len":
            agg = agg[:off] + bytes(max(0, off - len(agg)))
        else:
            {"pks": pks, "msgs": msgs, "agg": agg}[f][off:off + len(b)] = b
    return bytes(pks), bytes(msgs), bytes(agg)


def main():
    ref = Ref()
    rng = np.random.default_rng(20261019)
    out = {"sizes": list(SIZES), "aggregates": []}
    for n in SIZES:
        sigs, msgs, pks = ref.make_schnorr(n, rng) if n else (np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
        agg = ref.halfagg_aggregate(pks, msgs, sigs) if n else bytes(32)
        base = {"pks": pks.tobytes(), "msgs": msgs.tobytes(), "agg": agg}
        assert ref.halfagg_verify(base["pks"], base["msgs"], agg, n) == 1
        s = int.from_bytes(agg[32 * n:], "big")
        cases = []
        if n:
            i = int(rng.integers(0, n))
            bit = bytes([base["msgs"][32 * i + 5] ^ 0x10])
            cases.append(("message bit flipped", [["msgs", 32 * i + 5, bit.hex()]]))
            cases.append(("r_i >= p", [["agg", 32 * i, (P + 1).to_bytes(32, "big").hex()]]))
            cases.append(("r_i not an x coordinate", [["agg", 32 * i, not_an_x(rng).hex()]]))
            cases.append(("key does not parse", [["pks", 32 * i, not_an_x(rng).hex()]]))
            cases.append(("s >= n", [["agg", 32 * n, (N + (s % 1000)).to_bytes(32, "big").hex()]]))
            cases.append(("s off by one", [["agg", 32 * n, ((s + 1) % N).to_bytes(32, "big").hex()]]))
        else:
            cases.append(("n = 0, s = 1", [["agg", 0, (1).to_bytes(32, "big").hex()]]))
        if n >= 2:
            a, b = 0, n - 1
            cases.append(("two items swapped", [["msgs", 32 * a, base["msgs"][32 * b:32 * b + 32].hex()], ["msgs", 32 * b, base["msgs"][32 * a:32 * a + 32].hex()],
                                                ["pks", 32 * a, base["pks"][32 * b:32 * b + 32].hex()], ["pks", 32 * b, base["pks"][32 * a:32 * a + 32].hex()]]))
        cases.append(("32 bytes short", [["agg_len", 32 * n, ""]]))
        cases.append(("32 bytes long", [["agg_len", 32 * (n + 2), ""]]))
        rec = {"n": n, "pks": base["pks"].hex(), "objs": ref.xonly_objects(pks).tobytes().hex() if n else "", "msgs": base["msgs"].hex(), "sigs": sigs.tobytes().hex(),
               "agg": agg.hex(), "result": 1, "tampered": []}
        verdicts = [1]
        for name, patches in cases:
            p2, m2, a2 = apply(base, patches)
            v = max(0, ref.halfagg_verify(p2, m2, a2, n))           # (-1: a key does not parse; the engine's verdict is 0)
            t = {"name": name, "patches": patches, "result": v}
            touched = sorted({off // 32 for f, off, _ in patches if f == "pks"})
            if touched:
                keys = np.frombuffer(p2, np.uint8).reshape(-1, 32)
                valid = ref.xonly_valid(keys[touched])
                t["objs"] = [[k, (ref.xonly_objects(keys[k:k + 1]).tobytes() if ok else bytes(64)).hex()] for k, ok in zip(touched, valid)]
            rec["tampered"].append(t); verdicts.append(v)
        assert 1 in verdicts and 0 in verdicts, n
        assert verdicts[1:] == [0] * len(cases), (n, verdicts)      # (every tampering here is one the reference refuses)
        out["aggregates"].append(rec)
    # above the limit: one triple, 4 097 times
    sig, msg, pk = ref.make_schnorr(1, rng)
    agg = ref.halfagg_aggregate(np.tile(pk, (BIG, 1)), np.tile(msg, (BIG, 1)), np.tile(sig, (BIG, 1)))
    assert agg[:32 * BIG] == sig.tobytes()[:32] * BIG
    assert ref.halfagg_verify(np.tile(pk, (BIG, 1)), np.tile(msg, (BIG, 1)), agg, BIG) == 1
    out["repeated"] = {"count": BIG, "pk": pk.tobytes().hex(), "obj": ref.xonly_objects(pk).tobytes().hex(), "msg": msg.tobytes().hex(), "sig": sig.tobytes().hex(),
                       "s": agg[32 * BIG:].hex(), "result": 1}
    path = os.path.join(HERE, "halfagg_batch_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
