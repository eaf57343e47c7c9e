"""Inputs shared by tests/test_cpu_ring_joint.py and tests/test_gpu_ring_joint.py: the step list of the ring form (ecmult.h,
ecmult_ring_tables + ecmult_ring_step), R = e*C + s*G + f*G."""
import numpy as np

from tests.refapi import G_XY, N
from tests.test_cpu_oracle import LAMBDA

# the multipliers e named one by one.  A step on one of them may hand back (return 0, the caller's fallback gives the result) only where the
# separate form (S2K_RING_JOINT=0) hands back too: on the host emulation it completes every one of them, so the allowance is empty
# (tests/test_cpu_ring_joint.py checks both forms against it).
LISTED_E = [1, 2, 3, N - 1, N - 2, LAMBDA, LAMBDA + 1, LAMBDA - 1, 2**64, 2**128 + 1, 2**128 - 1]
HANDBACK_ALLOWED = ()


def b32(v):
    return int(v).to_bytes(32, "big")


def split_bound_scalars():
    # scalars_near_split_bounds, their negations and neighbours.  Imported, not copied, from a module of the GPU tier: that works in the CPU
    # tier because the module imports only json, os, numpy, pytest and tests.refapi at module level (torch inside its tests)
    from tests.test_gpu_split_bounds import _scalars
    return _scalars()


def step_list(ref, seed=9100, n_random=64):
    """(C (n, 64), e, s, f (n, 32) uint8, kind list): kind 'bound' / 'listed' / 'random' per row"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(G_XY, np.uint8)
    pool = [np.frombuffer(ref.rand_point(rng), np.uint8) for _ in range(8)] + [g]
    es = [(v, "bound") for v in split_bound_scalars()] + [(v, "listed") for v in LISTED_E]
    es += [(int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "big") % N or 1, "random") for _ in range(n_random)]
    C = np.stack([pool[rng.integers(0, len(pool))] for _ in es])
    e = np.stack([np.frombuffer(b32(v), np.uint8) for v, _ in es])
    s = rng.integers(0, 256, (len(es), 32), dtype=np.uint8); f = rng.integers(0, 256, (len(es), 32), dtype=np.uint8)
    s[:, 0] &= 0x7F; f[:, 0] &= 0x7F                          # below n: the device reads them without reduction flags
    return C, e, s, f, [k for _, k in es]


def reference(ref, C, e, s, f):
    sf = np.stack([np.frombuffer(b32((int.from_bytes(s[i].tobytes(), "big") + int.from_bytes(f[i].tobytes(), "big")) % N), np.uint8) for i in range(len(e))])
    return ref.ecmult_batch(C, e, ng=sf)
