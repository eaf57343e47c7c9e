#!/usr/bin/env python3
"""Writes tests/golden/ecdsa_wycheproof.json from the reference's *data file* src/wycheproof/ecdsa_secp256k1_sha256_bitcoin_test.json
(463 vectors under 99 keys; the test that reads it in the reference is src/tests.c:7804-7830).

Run in the build container (needs the reference tree and oracle/_ref):   python tests/golden/make_ecdsa_golden.py
Stored: the deduplicated 65-byte keys and, per vector, [tcId, key index, SHA-256 of the message, signature, verdict].  The verdict is
RECOMPUTED by running the reference (parse_der && verify, as its own test does) and must equal the file's `result`."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("S2K_REFERENCE", "/root/reference")


def main():
    from tests.ecdsa_ref import EcdsaRef
    ref = EcdsaRef()
    src = json.load(open(os.path.join(REF, "src", "wycheproof", "ecdsa_secp256k1_sha256_bitcoin_test.json")))
    keys, index, vectors = [], {}, []
    for g in src["testGroups"]:
        k = g["publicKey"]["uncompressed"]
        if k not in index:
            index[k] = len(keys); keys.append(k)
        pk = ref.pubkey_parse(bytes.fromhex(k))
        assert pk is not None
        for t in g["tests"]:
            h = hashlib.sha256(bytes.fromhex(t["msg"])).digest()
            so = ref.sig_parse_der(bytes.fromhex(t["sig"]))
            verdict = 0 if so is None else ref.verify_obj(so, h, pk)
            assert verdict == (t["result"] == "valid"), t["tcId"]
            vectors.append([t["tcId"], index[k], h.hex(), t["sig"], verdict])
    assert len(vectors) == src["numberOfTests"]
    out = os.path.join(HERE, "ecdsa_wycheproof.json")
    with open(out, "w") as f:
        f.write('{"source": "src/wycheproof/ecdsa_secp256k1_sha256_bitcoin_test.json", "fields": ["tcId", "key", "sha256(msg)", "sig (DER)", "verdict"],\n')
        f.write(' "keys": [\n' + ",\n".join('  "%s"' % k for k in keys) + "\n ],\n")
        f.write(' "vectors": [\n' + ",\n".join("  " + json.dumps(v) for v in vectors) + "\n ]}\n")
    print(out, len(keys), "keys,", len(vectors), "vectors,", sum(v[4] for v in vectors), "valid,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
