"""GPU tier: the ring form with its joint table (csrc/ecmult.h, S2K_RING_JOINT) on the device -- ecmult_ring_tables + ecmult_ring_step through
prim 40 of tests/gpu_prims at one wavefront, one wavefront plus a lone lane and three wavefronts plus a lone lane, and whole 64-bit proofs
through k_rp_rings_shared with two cached generators -- against the unmodified reference."""
import ctypes
import os

import numpy as np
import pytest

from tests.refapi import GENERATOR_H
from tests.ring_joint_cases import reference, step_list

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RTAB_WORDS, RAW_WAVE_WORDS, PTAB_WORDS = 528, 2 * 16 * 27 * 64, 544          # S2K_RTAB_WORDS, S2K_RRAW_WAVE_WORDS, S2K_PTAB_WORDS (csrc/ecmult.h)


@pytest.fixture(scope="module")
def lanes(ref):
    """193 lanes: the step list first (split-bound scalars, the listed e, 64 random triples), random triples behind it; one reference run"""
    C, e, s, f, kinds = step_list(ref, n_random=64)
    n = len(kinds)
    assert n <= 193
    C2, e2, s2, f2, k2 = step_list(ref, seed=9200, n_random=193)
    rnd = [i for i, k in enumerate(k2) if k == "random"][:193 - n]
    C = np.concatenate([C, C2[rnd]]); e = np.concatenate([e, e2[rnd]]); s = np.concatenate([s, s2[rnd]]); f = np.concatenate([f, f2[rnd]])
    kinds = kinds + ["random"] * len(rnd)
    want, winf = reference(ref, C, e, s, f)
    assert len(kinds) == 193 and not winf.any()
    return C, e, s, f, kinds, want


def _prim40(engine, n, A, b):
    import torch
    lib = ctypes.CDLL(os.path.join(HERE, "gpu_prims", "libs2k_gpuprims.so"))
    gsz = ctypes.c_size_t(0)
    gtab = engine._lib.s2k_engine_gtable(engine._h, ctypes.byref(gsz))
    waves = (n + 63) // 64                                                   # a started wavefront has its whole parking area
    scratch_words = n * RTAB_WORDS + waves * RAW_WAVE_WORDS + n * PTAB_WORDS + 64
    dev = lambda x: torch.tensor(np.ascontiguousarray(x, np.uint8).reshape(-1)).cuda()
    ta, tb = dev(A), dev(b)
    out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"); flag = torch.zeros(n + scratch_words, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.s2k_test_prim(40, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(flag.data_ptr()), ctypes.c_void_p(ta.data_ptr()), ctypes.c_void_p(tb.data_ptr()),
                             None, ctypes.c_void_p(gtab), n) == 1
    return out.cpu().numpy().reshape(n, 64), flag.cpu().numpy()[:n]


@pytest.mark.parametrize("n", [64, 65, 193])
def test_ring_form_lanes(engine, lanes, n):
    """the LAST n lanes of the 193 for n = 64, 65 put random triples only into whole wavefronts; n = 193 holds the whole step list"""
    C, e, s, f, kinds, want = (x[193 - n:] for x in lanes)
    got, flag = _prim40(engine, n, C, np.concatenate([e, s, f], axis=1))
    assert ((flag & 1) == 0).all()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))          # (with the caller's fallback where a wavefront handed back)
    done = (flag >> 1) == 1
    for w in range((n + 63) // 64):
        if all(k == "random" for k in kinds[64 * w:64 * w + 64]):
            assert done[64 * w:64 * w + 64].all(), w


def test_step_list_lanes_first(engine, lanes):
    """n = 65 and 64 once more with the step list in front: the split-bound scalars and the listed e fill the first wavefront"""
    for n in (64, 65):
        C, e, s, f, kinds, want = (x[:n] for x in lanes)
        got, flag = _prim40(engine, n, C, np.concatenate([e, s, f], axis=1))
        assert ((flag & 1) == 0).all() and (got == want).all()


def test_whole_proofs_two_cached_generators(engine, ref):
    """65 reference-signed proofs over H and 65 over a second generator, both with cached tables: 64 of min_bits = 64 and one of min_bits = 5,
    exp 2, min_value 17 per set, one proof of each set with a flipped bit"""
    rng = np.random.default_rng(9300)
    gen2 = ref.rand_point(rng)
    for gen in (GENERATOR_H, gen2):
        engine.cache_generator(gen)
        rows = lambda k: np.frombuffer(gen * k, np.uint8).reshape(k, 64).copy()
        c1, p1, g1, _ = ref.make_rangeproofs(64, rng, min_bits=64, gens64=rows(64))
        c2, p2, g2, _ = ref.make_rangeproofs(1, rng, min_bits=5, exp=2, min_value=17, gens64=rows(1))
        C = np.concatenate([c1, c2]); P = p1 + p2; G = np.concatenate([g1, g2])
        bad = int(rng.integers(0, 64))
        q = bytearray(P[bad]); q[len(q) // 2 + 7] ^= 0x10; P[bad] = bytes(q)
        e_res, e_mn, e_mx = ref.rangeproof_verify_many(C, P, G, threads=8)
        assert e_res.sum() == 64 and e_res[bad] == 0
        res, mn, mx = engine.rangeproof_verify_batch(C, P, G)
        hb = engine.rp_handback()
        assert np.array_equal(res, e_res) and np.array_equal(mn, e_mn) and np.array_equal(mx, e_mx)
        assert hb[0] > 0 and hb[2] == 0 and hb[3] == 0, hb                   # served by the shared-generator form, nothing handed back
        # the valid proofs alone: no hand-back either
        keep = [i for i in range(65) if i != bad]
        res, mn, mx = engine.rangeproof_verify_batch(C[keep], [P[i] for i in keep], G[keep])
        hb = engine.rp_handback()
        assert res.all() and hb[0] > 0 and hb[1] == 0 and hb[2] == 0 and hb[3] == 0, hb
