"""GPU tier: the construction of the three-base ring table with prefix products formed from the parked inputs (csrc/ecmult.h:
ecmult_ring3_tables) on the device through tests/gpu_prims/libs2k_ring_triple_prims.so at 65 lanes -- one full wavefront plus a lone lane,
the smallest shape where the interleaved columns and a partly filled wavefront both occur.  The parking areas are pre-filled with a
pattern and guard words sit around every region: no word at or above W x 64 of a wavefront's area is touched, every lane's 512 table words
are the host emulation's for the same C, and the points are the reference's."""
import ctypes
import os

import numpy as np
import pytest

from tests.ring_joint_cases import reference, step_list
from tests.test_cpu_ring_table_prefix import PARK_WORDS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RTAB_WORDS, RAW_WAVE_WORDS, PTAB_WORDS = 528, 2 * 16 * 27 * 64, 544          # S2K_RTAB_WORDS, S2K_RRAW_WAVE_WORDS, S2K_PTAB_WORDS (csrc/ecmult.h)
GUARD_WORDS, GUARD, PATTERN = 64, 0xA5C3961E, 0x5EED7AB1
N_LANES = 65


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "gpu_prims", "libs2k_ring_triple_prims.so")
    assert os.path.exists(path), "tests/gpu_prims/libs2k_ring_triple_prims.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.s2k_test_ring3.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] * 5 + [ctypes.c_int]
    out = (ctypes.c_int * 3)()
    L.s2k_test_ring3_sizes(out)
    assert list(out) == [RTAB_WORDS, RAW_WAVE_WORDS, PTAB_WORDS]
    return L


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_ring_table_prefix_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_ring_table_prefix_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = ctypes.CDLL(path)
    L.emu_r3p_table_of.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


@pytest.fixture(scope="module")
def run(lib, engine, ref):
    """one launch of 65 lanes with random triples -> everything the tests look at"""
    import torch
    C, e, s, f, kinds = step_list(ref, seed=9700, n_random=N_LANES)
    rnd = [i for i, k in enumerate(kinds) if k == "random"]
    assert len(rnd) == N_LANES
    C, e, s, f = C[rnd], e[rnd], s[rnd], f[rnd]
    want, winf = reference(ref, C, e, s, f)
    assert not winf.any()
    n, waves = N_LANES, 2
    gsz = ctypes.c_size_t(0)
    gtab = engine._lib.s2k_engine_gtable(engine._h, ctypes.byref(gsz))
    raw_stride = RAW_WAVE_WORDS + GUARD_WORDS
    sizes = [n * RTAB_WORDS] + [RAW_WAVE_WORDS] * waves + [n * PTAB_WORDS]
    starts, total = [], GUARD_WORDS
    for sz in sizes:
        starts.append(total); total += sz + GUARD_WORDS
    assert starts[2] == starts[1] + raw_stride
    host = np.zeros(total, np.uint32)
    guards = [slice(0, GUARD_WORDS)] + [slice(st + sz, st + sz + GUARD_WORDS) for st, sz in zip(starts, sizes)]
    for g in guards:
        host[g] = GUARD
    for w in range(waves):
        host[starts[1 + w]:starts[1 + w] + RAW_WAVE_WORDS] = PATTERN
    dev = lambda x: torch.tensor(np.ascontiguousarray(x, np.uint8).reshape(-1)).cuda()
    ta, tb = dev(C), dev(np.concatenate([e, s, f], axis=1))
    scratch = torch.tensor(host.view(np.int32)).cuda()
    out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"); flag = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.s2k_test_ring3(out.data_ptr(), flag.data_ptr(), ta.data_ptr(), tb.data_ptr(), gtab, scratch.data_ptr(), total, starts[0], starts[1], raw_stride, starts[-1], n) == 1
    after = scratch.cpu().numpy().view(np.uint32)
    return dict(C=C, want=want, got=out.cpu().numpy().reshape(n, 64), flag=flag.cpu().numpy(), after=after, guards=guards, starts=starts, sizes=sizes)


def test_guards_are_intact(run):
    for k, g in enumerate(run["guards"]):
        assert (run["after"][g] == GUARD).all(), ("guard", k, np.nonzero(run["after"][g] != GUARD)[0][:8])


def test_nothing_at_or_above_w_is_touched(run):
    """word w of lane l of a wavefront's area is at w * 64 + l: everything from W * 64 on still holds the pattern, in the full wavefront and in
    the one with a lone lane; below it the full wavefront has overwritten its columns and the lone lane only column 0"""
    for w in range(2):
        area = run["after"][run["starts"][1 + w]:run["starts"][1 + w] + RAW_WAVE_WORDS].reshape(-1, 64)
        assert (area[PARK_WORDS:] == PATTERN).all(), (w, np.nonzero((area[PARK_WORDS:] != PATTERN).any(axis=1))[0][:8] + PARK_WORDS)
        assert (area[PARK_WORDS - 1] != PATTERN).any(), w                    # W is the map's size, not an upper bound on it
    lone = run["after"][run["starts"][2]:run["starts"][2] + RAW_WAVE_WORDS].reshape(-1, 64)
    assert (lone[:, 1:] == PATTERN).all()


def test_table_words_equal_the_host_emulation(run, emu):
    """the 32 sectors are normalised coordinates on the Z  za z1 z2 D1 D2, which the host forms from the same C by the same doublings"""
    C = run["C"]
    rtab = run["after"][run["starts"][0]:run["starts"][0] + run["sizes"][0]].reshape(N_LANES, RTAB_WORDS)
    for i in range(N_LANES):
        words = np.zeros(520, np.uint32)
        assert emu.emu_r3p_table_of(words.ctypes.data, C[i].tobytes(), PARK_WORDS) == 1
        assert np.array_equal(rtab[i, :512], words[:512]), (i, np.nonzero(rtab[i, :512] != words[:512])[0][:8])


def test_points_equal_the_reference(run):
    assert ((run["flag"] & 1) == 0).all() and ((run["flag"] >> 1) == 1).all(), run["flag"]          # random triples: completed, nothing handed back
    assert (run["got"] == run["want"]).all(), np.nonzero((run["got"] != run["want"]).any(axis=1))
