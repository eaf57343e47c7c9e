#!/usr/bin/env python3
"""Writes tests/golden/whitelist_vectors.json: the whitelist edge list of tests/whitelist_ref.py at list lengths <= 15, as recorded inputs
(serialised signature, the two key lists and the sub key as 64-byte secp256k1_pubkey objects) and verdicts.

Run in the build container (needs oracle/_ref):   python tests/golden/make_whitelist_golden.py
The verdict of every vector is what secp256k1_whitelist_signature_parse && secp256k1_whitelist_verify of the reference returned when the
file was written; the three all-zero key objects are marked "engine only" (the reference is not asked: it calls its illegal-argument
callback there) and carry the engine's contract, 0."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    from tests.whitelist_ref import WhitelistRef, edge_cases
    cases = edge_cases(WhitelistRef(), with_255=False)
    out = os.path.join(HERE, "whitelist_vectors.json")
    with open(out, "w") as f:
        f.write('{"source": "tests/whitelist_ref.py edge_cases(with_255=False)", "fields": ["name", "sig", "online", "offline", "sub", "verdict"],\n')
        f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps([n, s.hex(), on.hex(), off.hex(), sub.hex(), v]) for n, s, on, off, sub, v in cases) + "\n ]}\n")
    print(out, len(cases), "vectors,", sum(c[5] for c in cases), "valid,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
