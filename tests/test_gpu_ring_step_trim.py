"""GPU tier: the signed-accumulator forms of the six-base ring step (csrc/group.h: gej_dblneg_ring, gej_rsub_ge_ring, gez_add_ge_ring)
on the device through tests/gpu_prims/ring_step_trim_prims.hip, one wavefront and one wavefront plus a lone lane, on the extreme-magnitude
rows of tests/test_cpu_ring_step_trim.py, limb for limb against the host build of the same lines; and k_rp_rings_shared, which runs them,
on 3 and on 65 reference-signed 64-bit proofs: verdict, minimum and maximum are the reference's and nothing is handed back."""
import ctypes
import os

import numpy as np
import pytest

from tests.refapi import GENERATOR_H
from tests.test_cpu_ring_step_trim import FORMS, form_cases, run_form

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KIND = {"dbl": 0, "dbl_nx": 1, "rsub": 2, "gez": 3}
OUT_WORDS = 37                                          # TRIM_OUT_WORDS of the prims file: up to 36 limbs and the same-x flag


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "gpu_prims", "libs2k_ring_step_trim_prims.so")
    assert os.path.exists(path), "tests/gpu_prims/libs2k_ring_step_trim_prims.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    import torch  # noqa: F401      (first: the library then binds to the HIP runtime torch has mapped -- secp256k1_zkp_amd/_native.py: load)
    L = ctypes.CDLL(path)
    L.s2k_test_trim_forms.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    return L


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_step_trim_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_step_trim_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.emu_trim_dbl.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
    L.emu_trim_rsub.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    L.emu_trim_gez.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def host_rows(emu):
    """per form: the 65 input rows (the case list, repeated from its start) and the host's limbs and flag for each"""
    out = {}
    for name in FORMS:
        cases = form_cases(name)
        rows = cases[np.arange(65) % len(cases)]
        res = [run_form(emu, name, r) for r in rows]
        out[name] = (rows, np.stack([r[0] for r in res]), np.array([r[2] & 1 for r in res], np.uint32))
    return out


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("name", list(FORMS))
def test_forms_limb_for_limb(lib, host_rows, name, n):
    import torch
    rows, want, wflag = host_rows[name]
    tin = torch.tensor(np.ascontiguousarray(rows[:n]).view(np.int32).reshape(-1)).cuda()
    tout = torch.full((n * OUT_WORDS + 64,), -1, dtype=torch.int32, device="cuda")          # 64 words behind the last item stay untouched
    torch.cuda.synchronize()
    assert lib.s2k_test_trim_forms(tout.data_ptr(), n * OUT_WORDS, tin.data_ptr(), tin.numel(), KIND[name], n) == 1
    got = tout.cpu().numpy().view(np.uint32)
    assert (got[n * OUT_WORDS:] == 0xFFFFFFFF).all()
    got = got[:n * OUT_WORDS].reshape(n, OUT_WORDS)
    k = want.shape[1]
    assert np.array_equal(got[:, :k], want[:n]), np.nonzero((got[:, :k] != want[:n]).any(axis=1))[0][:8]
    assert np.array_equal(got[:, 36], wflag[:n])


def test_buffers_too_small_are_refused(lib):
    assert lib.s2k_test_trim_forms(None, 65 * OUT_WORDS - 1, None, 65 * 54, 3, 65) == -1
    assert lib.s2k_test_trim_forms(None, 65 * OUT_WORDS, None, 65 * 54 - 1, 3, 65) == -1
    assert lib.s2k_test_trim_forms(None, 65 * OUT_WORDS, None, 65 * 54, 4, 65) == -1


@pytest.mark.parametrize("n", [3, 65])
def test_whole_proofs_through_the_shared_kernel(engine, ref, n):
    """n proofs of min_bits = 64 over H (cached table), one with a flipped bit"""
    assert engine._lib.s2k_ring_six() == 1
    rng = np.random.default_rng(9960 + n)
    engine.cache_generator(GENERATOR_H)
    rows = np.frombuffer(GENERATOR_H * n, np.uint8).reshape(n, 64).copy()
    C, P, G, _ = ref.make_rangeproofs(n, rng, min_bits=64, gens64=rows)
    P = list(P)
    bad = int(rng.integers(0, n))
    q = bytearray(P[bad]); q[len(q) // 2 + 7] ^= 0x10; P[bad] = bytes(q)
    e_res, e_mn, e_mx = ref.rangeproof_verify_many(C, P, G, threads=8)
    assert e_res.sum() == n - 1 and e_res[bad] == 0
    res, mn, mx = engine.rangeproof_verify_batch(C, P, G)
    hb = engine.rp_handback()
    assert np.array_equal(res, e_res) and np.array_equal(mn, e_mn) and np.array_equal(mx, e_mx)
    assert hb[0] > 0 and hb[2] == 0 and hb[3] == 0, hb                       # served by the shared-generator form, nothing handed back
