"""GPU: where the adaptor family places an item in a batch (csrc/engine_core.hip: secp256k1_ecdsa_adaptor_verify_batch_group;
csrc/engine_lanes.h: lanes_run; csrc/engine_adaptor.hip).  Group shares that start at lo > 0 and launches that start at i0 > 0, at every
key width; s2k_ecmult2_batch over several launches.  The pool, the points and the helpers are those of tests/test_gpu_adaptor.py; the
verdicts are the pool's (the Python model's), the points' results the reference's.  tests/batch_edges.py asserts before every call that
the batch could show a wrong stride or a dropped offset."""
import ctypes

import numpy as np
import pytest

from tests import adaptor_ref as A
from tests import batch_edges as E
from tests.test_gpu_adaptor import _arrays, _dev, _names, _take, _verify_dev, points, pool  # noqa: F401  (pool, points: fixtures)

pytestmark = pytest.mark.gpu

GROUP_SIZES = (1, 2, 3, 4, 5, 65, 257, 599)


@pytest.fixture(scope="module")
def groups():
    """three engines on device 0 (shares start at n/3 and 2n/3, and are empty below three items), and two engines on two devices where
    there are two"""
    import torch
    from secp256k1_zkp_amd import Group
    made = []
    try:
        made.append(Group([0, 0, 0]))
        made.append(Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0]))
        yield made
    finally:
        for g in made:
            g.close()


def _period(pool, fmt):
    """after how many kept items a batch cut cyclically from the pool repeats itself in pk_format fmt"""
    return sum(1 for it in pool if A.keys_in_format(it, fmt) is not None)


def _split_ok(what, pool, fmt, bounds, sigs, pks, msgs, eks, exp, both=True):
    E.check(what, bounds, dict(sigs=sigs, pks=pks, msgs=msgs, eks=eks), exp, period=_period(pool, fmt), both=both)


def test_group_shares(groups, pool):
    """groups of three and of two engines: every share but the first starts at lo > 0, where the `_group` form adds 162 * lo, 32 * lo
    and pkb * lo (33, 64 or 65 bytes per key, on two key arrays) to the caller's arrays.  1 .. 5 items leave shares empty or one item
    long; 599 items put the starts at 199 and 399 (at 299), which the pool's period does not divide (584 of them have an object form:
    194 and 389, 292, against a period of 195; tests/batch_edges.py asserts it).  The verdicts are the pool's."""
    for fmt in (0, 1, 2):
        for n in GROUP_SIZES if fmt == 0 else (599, 4):
            items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, n, start=7), fmt)
            m = len(items)
            assert m == n if fmt == 0 else m >= (560 if n == 599 else n - 1)              # (an item whose flipped bit broke a key has no object form)
            for g in groups:
                _split_ok((fmt, n, len(g)), pool, fmt, E.share_starts(m, len(g)), sigs, pks, msgs, eks, exp, both=m >= 65)
                got = g.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
                assert np.array_equal(got, exp), (fmt, n, len(g), np.flatnonzero(got != exp)[:8], _names(items, got, exp)[:4])


def test_group_argument_checks(groups, pool):
    """a NULL array or a pk_format out of range through the `_group` form: 0 with the argument status, and nothing marked valid"""
    g = groups[0]; L = g._lib
    items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, 6), 0)
    res = np.full(6, 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(sigs), p(pks), p(msgs), p(eks), 0, 6]
    assert L.secp256k1_ecdsa_adaptor_verify_batch_group(g._h, *good) == 1 and np.array_equal(res, exp)
    for k in (0, 1, 2, 3, 4):
        a = list(good); a[k] = None; res[:] = 7
        assert L.secp256k1_ecdsa_adaptor_verify_batch_group(g._h, *a) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), k
    for fmt in (3, -1):
        a = list(good); a[5] = fmt; res[:] = 7
        assert L.secp256k1_ecdsa_adaptor_verify_batch_group(g._h, *a) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), fmt
    assert L.secp256k1_ecdsa_adaptor_verify_batch_group(g._h, None, None, None, None, None, 0, 0) == 1


def test_sub_range_launches_key_objects_and_full_keys(pool):
    """700 items (683 with an object form) on an engine whose launches take 256 and then 512 lanes, with keys of 64 and of 65 bytes:
    launch i0 reads pubkeys + pkb * i0 and enckeys + pkb * i0.  Host and _dev form, against the pool's verdicts."""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        for fmt in (1, 2):
            items, sigs, pks, msgs, eks, exp = _arrays(_take(pool, 700, start=3), fmt)
            m = len(items)
            assert m >= 660 and 0 < exp.sum() < m
            for lanes in (256, 512):
                _split_ok((fmt, lanes), pool, fmt, E.launch_starts(m, lanes), sigs, pks, msgs, eks, exp)
                eng.set_option(Engine.OPT_MAX_LANES, lanes)
                got = eng.ecdsa_adaptor_verify_batch(sigs, pks, msgs, eks, pk_format=fmt)
                assert np.array_equal(got, exp), (fmt, lanes, _names(items, got, exp)[:4])
                d_res = _verify_dev(eng, sigs, pks, msgs, eks, fmt)
                eng.sync()
                got = d_res.cpu().numpy()
                assert np.array_equal(got, exp), (fmt, lanes, "dev", _names(items, got, exp)[:4])
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_ecmult2_sub_range_launches(points):
    """s2k_ecmult2_batch and its _dev form on an engine whose launches take 256 lanes.  Every lane parks a Jacobian point behind the tables
    with the launch's own stride, launch i0 reads and writes every array at i0, and the last launch is partial.  All 1000 items (the
    special cases in the first and the third launch of four), items 100 .. 799 (in the first and the last of three), both with the
    infinity flags; items 142 .. 703, which hold no special case, with NULL flags.  Against the reference's results."""
    import torch
    from secp256k1_zkp_amd import Engine
    a_xy, na, b_xy, nb, a_inf, b_inf, exp, exp_inf = points
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        for lo, hi, with_flags in ((0, 1000, True), (100, 800, True), (142, 704, False)):
            sl = slice(lo, hi); n = hi - lo
            assert with_flags or not (exp_inf[sl].any() or a_inf[sl].any() or b_inf[sl].any())
            assert n % 256 and len(E.launch_starts(n, 256)) >= 2
            E.check((lo, hi), E.launch_starts(n, 256), dict(a=a_xy[sl], na=na[sl], b=b_xy[sl], nb=nb[sl]), 1 - exp_inf[sl], both=False)
            flags = {"a_inf": a_inf[sl], "b_inf": b_inf[sl]} if with_flags else {}
            r, inf = eng.ecmult2_batch(a_xy[sl], na[sl], b_xy[sl], nb[sl], **flags)
            assert np.array_equal(inf, exp_inf[sl]), (lo, hi, np.flatnonzero(inf != exp_inf[sl])[:8])
            assert np.array_equal(r, exp[sl]), (lo, hi, np.flatnonzero((r != exp[sl]).any(axis=1))[:8])
            d_r = torch.full((n, 64), 0xFF, dtype=torch.uint8, device="cuda:0"); d_inf = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
            eng.ecmult2_batch_dev(d_r, d_inf, _dev(a_xy[sl]), _dev(na[sl]), _dev(b_xy[sl]), _dev(nb[sl]), **{k: _dev(v) for k, v in flags.items()})
            eng.sync()
            inf, r = d_inf.cpu().numpy(), d_r.cpu().numpy()
            assert np.array_equal(inf, exp_inf[sl]), (lo, hi, "dev", np.flatnonzero(inf != exp_inf[sl])[:8])
            assert np.array_equal(r, exp[sl]), (lo, hi, "dev", np.flatnonzero((r != exp[sl]).any(axis=1))[:8])
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()
