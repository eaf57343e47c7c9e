"""GPU tier: the six-base form of the ring table (csrc/ecmult.h: ecmult_ring6_tables + ecmult_ring6_step) on the device through
tests/gpu_prims/ring_six_prims.hip at one wavefront, one wavefront plus a lone lane and three wavefronts plus a lone lane.  The parking
areas are pre-filled with a pattern and guard words sit around every region and every wavefront's area: no word at or above W x 64 of an
area is touched, every lane's 512 table words are the host emulation's for the same C, and the points are the reference's.  And whole
proofs through k_rp_rings_shared with two cached generators, against the unmodified reference, on the form the library is built with."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.refapi import GENERATOR_H
from tests.ring_joint_cases import reference, step_list
from tests.test_cpu_ring_six import PARK_WORDS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RTAB_WORDS, RAW_WAVE_WORDS, PTAB_WORDS = 528, 2 * 16 * 27 * 64, 544          # S2K_RTAB_WORDS, S2K_RRAW_WAVE_WORDS, S2K_PTAB_WORDS (csrc/ecmult.h)
GUARD_WORDS, GUARD, PATTERN = 64, 0xA5C3961E, 0x5EED7AB1


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "gpu_prims", "libs2k_ring_six_prims.so")
    assert os.path.exists(path), "tests/gpu_prims/libs2k_ring_six_prims.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.s2k_test_ring6.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] * 5 + [ctypes.c_int]
    out = (ctypes.c_int * 4)()
    L.s2k_test_ring6_sizes(out)
    assert list(out) == [RTAB_WORDS, RAW_WAVE_WORDS, PTAB_WORDS, PARK_WORDS]
    return L


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_six_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_six_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.emu_r6_table_words_of.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


@pytest.fixture(scope="module")
def lanes(ref, emu):
    """193 lanes: the step list first (split-bound scalars, the listed e, 64 random triples), random triples behind it; one reference run and
    one host table per lane"""
    C, e, s, f, kinds = step_list(ref, n_random=64)
    n = len(kinds)
    assert n <= 193
    C2, e2, s2, f2, k2 = step_list(ref, seed=9800, n_random=193)
    rnd = [i for i, k in enumerate(k2) if k == "random"][:193 - n]
    C = np.concatenate([C, C2[rnd]]); e = np.concatenate([e, e2[rnd]]); s = np.concatenate([s, s2[rnd]]); f = np.concatenate([f, f2[rnd]])
    kinds = kinds + ["random"] * len(rnd)
    want, winf = reference(ref, C, e, s, f)
    assert len(kinds) == 193 and not winf.any()
    words = np.zeros((193, 520), np.uint32)
    for i in range(193):
        assert emu.emu_r6_table_words_of(words[i].ctypes.data, C[i].tobytes(), PARK_WORDS) == 1
    return C, e, s, f, kinds, want, words


def _run(lib, engine, n, A, b):
    """-> (points (n, 64), flags (n,), rtab (n, 528), the parking areas (waves, 864, 64)); asserts that every guard word -- in front of and
    behind rtab, every single wavefront's parking area and ptab -- is what it was"""
    import torch
    gsz = ctypes.c_size_t(0)
    gtab = engine._lib.s2k_engine_gtable(engine._h, ctypes.byref(gsz))
    waves = (n + 63) // 64                                                   # a started wavefront has its whole parking area
    raw_stride = RAW_WAVE_WORDS + GUARD_WORDS                                # a guard between any two wavefronts' parking areas
    sizes = [n * RTAB_WORDS] + [RAW_WAVE_WORDS] * waves + [n * PTAB_WORDS]
    starts, total = [], GUARD_WORDS
    for sz in sizes:
        starts.append(total); total += sz + GUARD_WORDS
    assert all(starts[1 + w] == starts[1] + w * raw_stride for w in range(waves))
    host = np.zeros(total, np.uint32)
    guards = [slice(0, GUARD_WORDS)] + [slice(st + sz, st + sz + GUARD_WORDS) for st, sz in zip(starts, sizes)]
    for g in guards:
        host[g] = GUARD
    assert sum(g.stop - g.start for g in guards) + sum(sizes) == total
    for w in range(waves):
        host[starts[1 + w]:starts[1 + w] + RAW_WAVE_WORDS] = PATTERN
    dev = lambda x: torch.tensor(np.ascontiguousarray(x, np.uint8).reshape(-1)).cuda()
    ta, tb = dev(A), dev(b)
    scratch = torch.tensor(host.view(np.int32)).cuda()
    out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"); flag = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.s2k_test_ring6(out.data_ptr(), flag.data_ptr(), ta.data_ptr(), tb.data_ptr(), gtab, scratch.data_ptr(), total, starts[0], starts[1], raw_stride, starts[-1], n) == 1
    after = scratch.cpu().numpy().view(np.uint32)
    for k, g in enumerate(guards):
        assert (after[g] == GUARD).all(), ("guard", k, np.nonzero(after[g] != GUARD)[0][:8])
    areas = np.stack([after[starts[1 + w]:starts[1 + w] + RAW_WAVE_WORDS].reshape(-1, 64) for w in range(waves)])
    return out.cpu().numpy().reshape(n, 64), flag.cpu().numpy(), after[starts[0]:starts[0] + sizes[0]].reshape(n, RTAB_WORDS).copy(), areas


@pytest.mark.parametrize("n", [64, 65, 193])
def test_ring6_lanes(lib, engine, lanes, n):
    """the LAST n lanes of the 193 for n = 64, 65 put random triples only into whole wavefronts (which must complete without hand-back);
    n = 193 holds the whole step list"""
    C, e, s, f, kinds, want, words = (x[193 - n:] for x in lanes)
    got, flag, rtab, areas = _run(lib, engine, n, C, np.concatenate([e, s, f], axis=1))
    assert ((flag & 1) == 0).all()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))          # (with the caller's fallback where a wavefront handed back)
    done = (flag >> 1) == 1
    for w in range((n + 63) // 64):
        if all(k == "random" for k in kinds[64 * w:64 * w + 64]):
            assert done[64 * w:64 * w + 64].all(), w
    # the 32 sectors are normalised coordinates on the table's Z, which the host forms from the same C by the same doublings
    assert np.array_equal(rtab[:, :512], words[:, :512]), np.nonzero((rtab[:, :512] != words[:, :512]).any(axis=1))[0][:8]
    # word w of lane l of a wavefront's area is at w * 64 + l: everything from W * 64 on still holds the pattern, a lane that does not exist
    # leaves its column alone, and W is the map's size, not an upper bound on it
    for w, area in enumerate(areas):
        live = min(64, n - 64 * w)
        assert (area[PARK_WORDS:] == PATTERN).all(), (w, np.nonzero((area[PARK_WORDS:] != PATTERN).any(axis=1))[0][:8] + PARK_WORDS)
        assert (area[:, live:] == PATTERN).all(), w
        assert (area[PARK_WORDS - 1, :live] != PATTERN).any(), w


def test_step_list_lanes_first(lib, engine, lanes):
    """n = 65 once more with the step list in front: the split-bound scalars and the listed e fill the first wavefront"""
    C, e, s, f, kinds, want, words = (x[:65] for x in lanes)
    got, flag, rtab, areas = _run(lib, engine, 65, C, np.concatenate([e, s, f], axis=1))
    assert ((flag & 1) == 0).all() and (got == want).all()
    assert np.array_equal(rtab[:, :512], words[:, :512])


def test_regions_outside_the_scratch_are_refused(lib):
    """the entry point launches nothing when a region does not lie inside the buffer it was given"""
    assert lib.s2k_test_ring6(None, None, None, None, None, None, 65 * RTAB_WORDS, 0, 0, RAW_WAVE_WORDS, 0, 65) == -1
    assert lib.s2k_test_ring6(None, None, None, None, None, None, 1 << 30, 0, 0, RAW_WAVE_WORDS - 1, 0, 65) == -1          # areas that would overlap


def committed_default():
    """the default of S2K_RING_SIX as csrc/rangeproof.h sets it"""
    src = open(os.path.join(HERE, "..", "secp256k1_zkp_amd", "csrc", "rangeproof.h")).read()
    m = re.search(r"#ifndef S2K_RING_SIX\s*\n#define S2K_RING_SIX (\d+)", src)
    assert m
    return int(m.group(1))


def test_whole_proofs_two_cached_generators(engine, ref):
    """65 reference-signed proofs over H and 65 over a second generator, both with cached tables: 64 of min_bits = 64 and one of min_bits = 5,
    exp 2, min_value 17 per set, one proof of each set with a flipped bit; the library's rings kernel is built with the committed default of
    S2K_RING_SIX"""
    assert engine._lib.s2k_ring_triple() == 1
    assert engine._lib.s2k_ring_six() == committed_default()
    rng = np.random.default_rng(9900)
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
