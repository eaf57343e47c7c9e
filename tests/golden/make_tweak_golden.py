#!/usr/bin/env python3
"""Writes tests/golden/tweak_vectors.json: the tweak edge list of tests/tweak_ref.py and 64 seeded random items, as recorded inputs
(key in its format, tweak, the check form's tweaked32 and parity byte) with the reference's check verdict, add verdict and output key.

Run in the build container (needs oracle/_ref):   python tests/golden/make_tweak_golden.py
Every verdict and output key is what secp256k1_xonly_pubkey_tweak_add_check / secp256k1_xonly_pubkey_tweak_add /
secp256k1_ec_pubkey_tweak_add of the reference returned when the file was written; the all-zero key object is engine only (the reference
is not asked: it calls its illegal-argument callback there) and carries the engine's contract, 0.  null: the form does not apply (see
tests/tweak_ref.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

RANDOM_SEED = 4402


def main():
    from tests.tweak_ref import TweakRef, edge_cases, random_items, to_json
    ref = TweakRef()
    items = edge_cases(ref) + random_items(ref, 64, RANDOM_SEED)
    out = os.path.join(HERE, "tweak_vectors.json")
    with open(out, "w") as f:
        f.write('{"source": "tests/tweak_ref.py edge_cases() + random_items(64, %d)",\n' % RANDOM_SEED)
        f.write(' "fields": ["name", "key_format", "key", "tweak32", "tweaked32", "parity", "check_verdict", "add_verdict", "out64"],\n')
        f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps(r) for r in to_json(items)) + "\n ]}\n")
    print(out, len(items), "vectors,", sum(1 for i in items if i[6] == 1), "valid checks,", sum(1 for i in items if i[7] == 1), "valid adds,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
