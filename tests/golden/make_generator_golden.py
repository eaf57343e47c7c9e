#!/usr/bin/env python3
"""Writes tests/golden/generator_vectors.json: the generator edge list of tests/generator_ref.py and 64 seeded random items per entry
point (parse, serialize, generate, commit), as recorded inputs with the reference's verdict and output.

Run in the build container (needs oracle/_ref):   python tests/golden/make_generator_golden.py
Every verdict, and every output of an item with verdict 1, is what secp256k1_generator_parse / _serialize / _generate /
_generate_blinded / secp256k1_pedersen_commit of the reference gave when the file was written; where the verdict is 0 the output is the
engine's contract, zero bytes (see tests/generator_ref.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

RANDOM_SEED = 5502


def main():
    from tests.generator_ref import GeneratorRef, edge_cases, random_items, to_json
    ref = GeneratorRef()
    items = edge_cases(ref) + random_items(ref, 64, RANDOM_SEED)
    out = os.path.join(HERE, "generator_vectors.json")
    with open(out, "w") as f:
        f.write('{"source": "tests/generator_ref.py edge_cases() + random_items(64, %d)",\n' % RANDOM_SEED)
        f.write(' "fields": ["op", "name", "args", "verdict", "out"],\n')
        f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps(r) for r in to_json(items)) + "\n ]}\n")
    print(out, len(items), "vectors,", sum(1 for i in items if i[3] == 1), "with verdict 1,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
