#!/usr/bin/env python3
"""Writes tests/golden/pubkey_vectors.json: the public-key edge lists of tests/pubkey_ref.py and 64 seeded random items per call
(convert / negate, tweak_mul, combine), as recorded inputs with the reference's verdict and result object (the other five encodings,
the parity and the negation follow from the object by byte shuffling: tests/pubkey_ref.py derive_outs).

Run in the build container (needs oracle/_ref):   python tests/golden/make_pubkey_golden.py
Every verdict and output is what the reference's secp256k1_ec_pubkey_parse / _serialize / _negate / _tweak_mul / _combine and
secp256k1_xonly_pubkey_parse / _serialize / _from_pubkey returned when the file was written; the all-zero key object, the empty set and a
set with a key that does not load are engine only (the reference is not asked: it calls its illegal-argument callback there or has no
such input) and carry the engine's contract, 0 and zero bytes."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

RANDOM_SEED = 7704


def main():
    from tests.pubkey_ref import PubkeyRef, edge_cases, random_items, to_json
    ref = PubkeyRef()
    edge, rnd = edge_cases(ref), random_items(ref, 64, RANDOM_SEED)
    items = to_json({k: edge[k] + rnd[k] for k in edge})
    out = os.path.join(HERE, "pubkey_vectors.json")
    with open(out, "w") as f:
        f.write('{"source": "tests/pubkey_ref.py edge_cases() + random_items(64, %d); blobs: every distinct byte string once, rows name them by index",\n' % RANDOM_SEED)
        f.write(' "fields": {"convert": ["name", "in_format", "key", "verdict", "result object or null"],\n')
        f.write('            "tweak_mul": ["name", "key_format", "key", "tweak32", "verdict", "result object or null"],\n')
        f.write('            "combine": ["name", "key_format", "keys", "verdict", "result object or null"]},\n')
        f.write(' "vectors": {\n' + ",\n".join('  "%s": [\n' % k + ",\n".join("   " + json.dumps(r) for r in (v if k != "blobs" else [" ".join(v[i:i + 8]) for i in range(0, len(v), 8)])) + "\n  ]" for k, v in items.items()) + "\n }}\n")
    print(out, {k: len(v) for k, v in items.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
