"""GPU tier of the one-verdict BIP-340 batch verifier (engine_schnorr_all.hip): the seed against hashlib, the BIP-340 vectors, the
reference's signatures valid and corrupted in the batch shapes of the CPU tier (tests/schnorr_all_cases.py), cancelling changes,
coincident points, the empty batch, the `_dev` form on tensors and the C example.  Every host call is also held against the AND of the
per-item verifier on the same batch."""
import os
import subprocess

import numpy as np
import pytest

from tests import schnorr_all_cases as C
from tests import schnorr_all_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _call(engine):
    def call(s, m, k, msglen, pk_format, locate):
        s, m, k = (np.ascontiguousarray(x, np.uint8) for x in (s, m, k))
        out = engine.schnorrsig_verify_all(s, m, k, msglen=msglen, pk_format=pk_format, locate=locate, want_seed=True)
        v, res, seed = (out[0], out[1], out[2]) if locate else (out[0], None, out[1])
        n = s.size // 64
        per_item = engine.schnorrsig_verify_batch(s, m, k, msglen=msglen, pk_format=pk_format) if n else np.ones(0, np.int32)
        assert v == int(per_item.all()), "the verdict is not the AND of the per-item verdicts"
        if locate:
            assert res.tolist() == (per_item.tolist() if not v else [1] * n)
        assert seed == R.seed(s, m, k, msglen, pk_format)
        return v, res, seed
    return call


@pytest.mark.parametrize("msglen", [0, 32, 33])
@pytest.mark.parametrize("n", [1, 16, 17, 256, 257, 4097])
def test_seed_against_hashlib(engine, n, msglen):
    """random bytes: the verdict is 0, the seed is the derivation's (tree-level boundaries up to three levels)"""
    s, m, k = C.random_batch(n, msglen)
    v, seed = engine.schnorrsig_verify_all(s, m, k, msglen=msglen, want_seed=True)
    assert v == 0 and seed == R.seed(s, m, k, msglen, 0)


def test_bip340_vectors(engine):
    C.check_vectors(_call(engine))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_valid_batches(engine, ref, n):
    C.check_valid(_call(engine), ref, n)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_one_corruption(engine, ref, n):
    C.check_corrupted(_call(engine), ref, n, where=[n - 1] if n == 4097 else None)


@pytest.mark.parametrize("n", [2, 17, 65])
def test_cancelling_changes_are_caught(engine, ref, n):
    C.check_cancellation(_call(engine), ref, n)


def test_coincident_points(engine):
    C.check_coincident(_call(engine))


def test_empty_batch(engine):
    C.check_empty(_call(engine))


@pytest.mark.parametrize("pk_format", [0, 1])
def test_dev_form_on_tensors(engine, ref, pk_format):
    import torch
    dev = torch.device("cuda", 0)
    for n, spoil in ((257, None), (257, 100), (1, None), (17, 16)):
        s, m, k = (x.copy() for x in C.valid_batch(ref, n))
        if spoil is not None:
            s[spoil, 40] ^= 4
        keys = ref.xonly_objects(k) if pk_format else k
        want_v, want_seed = engine.schnorrsig_verify_all(s, m, keys, pk_format=pk_format, want_seed=True)
        assert want_v == int(spoil is None)
        d_s, d_m, d_k = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s, m, keys))
        d_v = torch.full((1,), -7, dtype=torch.int32, device=dev); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        engine.schnorrsig_verify_all_dev(d_v, d_s, d_m, d_k, pk_format=pk_format, seed_out=d_seed)
        engine.sync()
        assert int(d_v.cpu()[0]) == want_v and d_seed.cpu().numpy().tobytes() == want_seed
        d_v.fill_(-7); torch.cuda.synchronize()
        engine.schnorrsig_verify_all_dev(d_v, d_s, d_m, d_k, pk_format=pk_format)           # without the seed
        engine.sync()
        assert int(d_v.cpu()[0]) == want_v
        assert engine.last_ms(0) > 0 and engine.last_ms(1) > 0 and all(x >= 0 for x in engine.schnorr_all_last_split_ms())
    d_v = torch.full((1,), -7, dtype=torch.int32, device=dev); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device=dev)
    e = torch.zeros(0, dtype=torch.uint8, device=dev)
    engine.schnorrsig_verify_all_dev(d_v, e, e, e, pk_format=pk_format, seed_out=d_seed, n=0)
    engine.sync()
    assert int(d_v.cpu()[0]) == 1 and d_seed.cpu().numpy().tobytes() == bytes(32)


def test_batch_too_large(engine):
    """more terms than one sum indexes: refused as an illegal argument before anything is read"""
    from secp256k1_zkp_amd import Engine, S2KError, _native
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MSM_MAX_TERMS, 64)
        s, m, k = C.random_batch(32, 32)
        with pytest.raises(S2KError):
            eng.schnorrsig_verify_all(s, m, k)
        assert "batch too large" in _native.last_error() and eng._lib.s2k_last_status() == 2
        assert eng.schnorrsig_verify_all(s[:31], m[:31], k[:31]) == 0
    finally:
        eng.close()


def test_c_example(tmp_path, ref):
    """examples/schnorr_verify_all.c (gcc -std=c99) linked against the shared library"""
    exe = str(tmp_path / "schnorr_verify_all")
    libdir = os.path.join(ROOT, "secp256k1_zkp_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "schnorr_verify_all.c"), "-o", exe,
                    os.path.join(libdir, "libsecp256k1_zkp_amd.so"), "-Wl,-rpath," + libdir], check=True)
    s, m, k = (x.copy() for x in C.valid_batch(ref, 65))
    for spoil in (None, 64):
        if spoil is not None:
            m[spoil, 0] ^= 1
        (tmp_path / "items.bin").write_bytes(b"".join(k[i].tobytes() + m[i].tobytes() + s[i].tobytes() for i in range(65)))
        out = subprocess.run([exe, str(tmp_path / "items.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr)
        lines = out.stdout.strip().split("\n")
        assert lines[0] == "%d 65 %s" % (spoil is None, R.seed(s, m, k).hex())
        assert lines[1:] == ([] if spoil is None else ["invalid: 64"])
