"""GPU tier of the one-verdict BP++ norm-argument verifier (engine_bppp_all.hip): the batches of the CPU tier (tests/bppp_all_cases.py)
through the engine -- the seed against hashlib, the reference's proofs valid and corrupted, its 13 vectors, cancelling changes, coincident
points, infinity encodings, the empty batch -- the `_dev` form on tensors, locating failures, the engine's generator-table states and
the C example.  Every host call is also held against the AND of the per-item verifier on the same batch."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bppp_all_cases as C
from tests import bppp_all_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _call(engine):
    def call(batch, locate):
        out = engine.bppp_norm_product_verify_all(*batch, locate=locate, want_seed=True)
        v, res, seed = (out[0], out[1], out[2]) if locate else (out[0], None, out[1])
        n = batch[2].size // 32
        per_item = engine.bppp_norm_product_verify_batch(*batch) if n else np.ones(0, np.int32)
        assert v == int(per_item.all()), "the verdict is not the AND of the per-item verdicts"
        if locate:
            assert res.tolist() == (per_item.tolist() if not v else [1] * n)
        shape_ok = n and batch[3].shape[0] == batch[4] + batch[5].shape[1] and batch[4] > 0 and batch[0].shape[1] == 65 * C.n_rounds(batch[4], batch[5].shape[1]) + 64
        assert seed == (R.seed(*batch) if shape_ok else bytes(32))
        return v, res, seed
    return call


@pytest.fixture(scope="module")
def tw(ref):
    from tests import tweak_ref
    return tweak_ref.TweakRef()


@pytest.mark.parametrize("shape,n", [((4, 4), 1), ((4, 4), 17), ((4, 4), 257), ((64, 8), 16), ((64, 8), 33)])
def test_seed_against_hashlib(engine, shape, n):
    """random bytes: the verdict is 0, the seed is the derivation's"""
    batch = C.random_batch(shape, n)
    v, seed = engine.bppp_norm_product_verify_all(*batch, want_seed=True)
    assert v == 0 and seed == R.seed(*batch)


@pytest.mark.parametrize("shape,n", [((4, 4), n) for n in (1, 2, 63, 64, 65, 257)] + [(s, n) for s in ((64, 8), (2, 8), (1, 1), (256, 1)) for n in (1, 17, 64)])
def test_valid_batches(engine, ref, shape, n):
    C.check_valid(_call(engine), ref, shape, n)


@pytest.mark.parametrize("shape,n", [((4, 4), n) for n in (1, 2, 63, 64, 65, 257)] + [(s, n) for s in ((64, 8), (2, 8)) for n in (1, 17, 64)])
def test_one_corruption(engine, ref, shape, n):
    C.check_corrupted(_call(engine), ref, shape, n, where=[n - 1] if n > 17 else None)


@pytest.mark.parametrize("shape,n", [((1, 1), 17), ((256, 1), 17), ((256, 1), 64)])
def test_one_corruption_other_shapes(engine, ref, shape, n):
    # (1, 1) has no round: no X or R, and no challenge is drawn, so its transcript is never read
    kinds = {"n", "l", "rho = 0", "the commitment"} | ({"an X byte", "the sign byte of a round", "a transcript state word"} if shape[0] > 1 else set())
    C.check_corrupted(_call(engine), ref, shape, n, where=[n // 2], kinds=kinds)


def test_reference_vectors(engine, ref):
    C.check_vectors(_call(engine), ref)


@pytest.mark.parametrize("n", [2, 17, 65])
def test_cancelling_changes_are_caught(engine, ref, tw, n):
    C.check_cancellation(_call(engine), ref, tw, (4, 4), n)


def test_coincident_points(engine, ref):
    C.check_coincident(_call(engine), ref)


def test_infinity_encodings(engine, ref):
    C.check_infinity_encodings(_call(engine), ref)


def test_empty_batch_and_rejected_shape(engine, ref):
    C.check_empty(_call(engine))
    good = C.valid_batch(ref, (4, 4), 5)
    v, res, seed = _call(engine)((good[0], good[1], good[2], good[3], 2, good[5], good[6]), True)
    assert v == 0 and res.tolist() == [0] * 5 and seed == bytes(32)


def test_column_sum_takes_two_passes(engine, ref):
    """one proof more than a lane of the first pass folds"""
    from secp256k1_zkp_amd import _native
    emu = ctypes.CDLL(os.path.join(HERE, "host_emul", "libs2k_bppp_all_emu.so")); emu.emu_bppp_all_chunk.restype = ctypes.c_uint
    L = emu.emu_bppp_all_chunk()
    assert R.colsum_plan(L + 1, L) == [2, 1] and _native is not None
    C.check_valid(_call(engine), ref, (4, 4), L + 1)
    C.check_corrupted(_call(engine), ref, (4, 4), L + 1, where=[L], kinds={"l", "an R byte"})


def test_locate_two_broken_proofs(engine, ref):
    b = C.copy(C.valid_batch(ref, (64, 8), 33))
    b[0][4, 70] ^= 1; b[2][32, 0] ^= 1
    v, res = engine.bppp_norm_product_verify_all(*b, locate=True)
    assert v == 0 and [i for i in range(33) if not res[i]] == [4, 32]
    assert res.tolist() == ref.bppp_verify_many(*b).tolist()


def test_dev_form_on_tensors(engine, ref):
    import torch
    dev = torch.device("cuda", 0)
    for shape, n, spoil in (((64, 8), 64, None), ((64, 8), 64, 40), ((4, 4), 1, None), ((4, 4), 17, 16)):
        b = C.copy(C.valid_batch(ref, shape, n))
        if spoil is not None:
            b[0][spoil, 40] ^= 4
        proofs, trs, rhos, gens, g_len, cvs, commits = b
        want_v, want_seed = engine.bppp_norm_product_verify_all(*b, want_seed=True)
        assert want_v == int(spoil is None)
        d_p, d_t, d_r, d_g, d_c, d_m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (proofs, trs, rhos, gens, cvs, commits))
        d_v = torch.full((1,), -7, dtype=torch.int32, device=dev); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        engine.bppp_norm_product_verify_all_dev(d_v, d_p, proofs.shape[1], d_t, d_r, d_g, gens, g_len, d_c, cvs.shape[1], d_m, n, seed_out=d_seed)
        engine.sync()
        assert int(d_v.cpu()[0]) == want_v and d_seed.cpu().numpy().tobytes() == want_seed
        d_v.fill_(-7); torch.cuda.synchronize()
        engine.bppp_norm_product_verify_all_dev(d_v, d_p, proofs.shape[1], d_t, d_r, d_g, gens, g_len, d_c, cvs.shape[1], d_m, n)          # without the seed
        engine.sync()
        assert int(d_v.cpu()[0]) == want_v
        assert engine.last_ms(0) > 0 and engine.last_ms(1) > 0 and all(x >= 0 for x in engine.bppp_all_last_split_ms())
    d_v = torch.full((1,), -7, dtype=torch.int32, device=dev); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device=dev)
    engine.bppp_norm_product_verify_all_dev(d_v, None, 194, None, None, None, None, 4, None, 4, None, 0, seed_out=d_seed)
    engine.sync()
    assert int(d_v.cpu()[0]) == 1 and d_seed.cpu().numpy().tobytes() == bytes(32)


def test_engine_states(ref):
    """a fresh engine with no fixed-base table of the set; after the per-item verifier has built it; two sets in alternation"""
    from secp256k1_zkp_amd import Engine
    a, b = C.valid_batch(ref, (8, 2), 6), C.valid_batch(ref, (4, 4), 6)
    bad = C.copy(a); bad[0][3, 9] ^= 1
    eng = Engine(0)
    try:
        assert eng.bppp_norm_product_verify_all(*a) == 1 and eng.bppp_norm_product_verify_all(*bad) == 0               # no table yet
        assert eng.bppp_norm_product_verify_batch(*bad).tolist() == [1, 1, 1, 0, 1, 1]                                  # builds the table of a's set
        assert eng.bppp_norm_product_verify_all(*a) == 1 and eng.bppp_norm_product_verify_all(*bad) == 0
        for batch in (b, a, b, a):
            assert eng.bppp_norm_product_verify_all(*batch) == 1
            v, res = eng.bppp_norm_product_verify_all(*bad, locate=True)                                                # the locating call switches the table to a's set
            assert v == 0 and res.tolist() == [1, 1, 1, 0, 1, 1]
        g2 = a[3].copy(); g2[3] = g2[4]                                                                                 # same length, one generator replaced
        assert eng.bppp_norm_product_verify_all(a[0], a[1], a[2], g2, *a[4:]) == 0 and eng.bppp_norm_product_verify_all(*a) == 1
        g2[3, 0] = 7                                                                                                    # a generator that does not parse
        assert eng.bppp_norm_product_verify_all(a[0], a[1], a[2], g2, *a[4:]) == 0
    finally:
        eng.close()


def test_batch_too_large(ref):
    """more points than one sum indexes: refused as an illegal argument before anything is read"""
    from secp256k1_zkp_amd import Engine, S2KError, _native
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MSM_MAX_TERMS, 64)                          # (the option's smallest value)
        good = C.valid_batch(ref, (4, 4), 12)                                 # 8 generators + 5 points a proof + G: 69 terms
        with pytest.raises(S2KError):
            eng.bppp_norm_product_verify_all(*good)
        assert "batch too large" in _native.last_error() and eng._lib.s2k_last_status() == 2
        assert eng.bppp_norm_product_verify_all(*(x[:11] if k not in (3, 4) else x for k, x in enumerate(good))) == 1          # 64 terms
    finally:
        eng.close()


def test_c_example(tmp_path, ref):
    """examples/bppp_verify_all.c (gcc -std=c99) linked against the shared library"""
    exe = str(tmp_path / "bppp_verify_all")
    libdir = os.path.join(ROOT, "secp256k1_zkp_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "bppp_verify_all.c"), "-o", exe,
                    os.path.join(libdir, "libsecp256k1_zkp_amd.so"), "-Wl,-rpath," + libdir], check=True)
    b = C.copy(C.valid_batch(ref, (64, 8), 17))
    for spoil in (None, 16):
        if spoil is not None:
            b[5][spoil, 0, 0] ^= 1
        proofs, trs, rhos, gens, g_len, cvs, commits = b
        data = struct.pack("<4I", g_len, cvs.shape[1], proofs.shape[1], 17) + gens.tobytes()
        data += b"".join(proofs[i].tobytes() + trs[i].tobytes() + rhos[i].tobytes() + cvs[i].tobytes() + commits[i].tobytes() for i in range(17))
        (tmp_path / "batch.bin").write_bytes(data)
        out = subprocess.run([exe, str(tmp_path / "batch.bin")], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout[-500:], out.stderr)
        lines = out.stdout.strip().split("\n")
        assert lines[0] == "%d 17 %s" % (spoil is None, R.seed(*b).hex())
        assert lines[1:] == ([] if spoil is None else ["invalid: 16"])
