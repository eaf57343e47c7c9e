"""GPU: where the sign-to-contract family places an item in a batch (csrc/engine_core.hip: s2c_group_form; csrc/engine_lanes.h: lanes_run,
der_window; csrc/engine_s2c.hip).  Group shares that start at lo > 0 and launches that start at i0 > 0, at every signature, key and
opening width; the host commitments over several launches.  The pool and the helpers are those of tests/test_gpu_s2c.py; the verdicts
are the pool's (the Python model's), the commitments the model's.  tests/batch_edges.py asserts before every call that the batch could
show a wrong stride or a dropped offset."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from tests import batch_edges as E
from tests import s2c_ref as S
from tests.test_gpu_s2c import PK_BYTES, _both_dev, _commit, _dev, _host, _names, _take, pool  # noqa: F401  (pool: a fixture)

pytestmark = pytest.mark.gpu

GROUP_SIZES = (1, 2, 3, 4, 5, 65, 257, 599)
SPLIT_FORMATS = ((1, 1, 1), (2, 2, 0), (0, 1, 1))


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


@functools.lru_cache(maxsize=None)
def _in_format(item, sf, pf, of):
    """S.keys_in_format, each answer kept: the batches are cut from 200 items over and over, and an object form costs a square root"""
    return S.keys_in_format(item, sf, pf, of)


def _arrays(items, sf=0, pf=0, of=0):
    """tests/test_gpu_s2c.py's _arrays over the kept conversions: items that exist in this format combination -> dict: kept items, sigs
    (array, or list of byte strings for DER), msgs, pks, data, openings, expected commit and host verdicts"""
    kept, sigs, pks, ops = [], [], [], []
    for it in items:
        got = _in_format(it, sf, pf, of)
        if got is not None:
            kept.append(it); sigs.append(got[0]); pks.append(got[1]); ops.append(got[2])
    n = len(kept)
    arr = lambda bs, w: np.frombuffer(b"".join(bs), np.uint8).reshape(n, w).copy()      # noqa: E731
    return dict(items=kept, sigs=sigs if sf == 2 else arr(sigs, 64), msgs=arr([x[2] for x in kept], 32), pks=arr(pks, PK_BYTES[pf]), data=arr([x[4] for x in kept], 32),
                ops=arr(ops, 64 if of else 33), commit=np.array([x[6] for x in kept], np.int32), host=np.array([x[7] for x in kept], np.int32), fmt=(sf, pf, of), n=n)


def _period(pool, fmt):
    """after how many kept items a batch cut cyclically from the pool repeats itself in the format combination"""
    return sum(1 for it in pool if _in_format(it, *fmt) is not None)


def _split_ok(what, pool, a, bounds, both=True):
    """tests/batch_edges.py on both verifiers' inputs: the commitment check reads neither message nor key"""
    E.check(what, bounds, dict(sigs=a["sigs"], data=a["data"], ops=a["ops"]), a["commit"], period=_period(pool, a["fmt"]), both=both)
    E.check(what, bounds, dict(sigs=a["sigs"], msgs=a["msgs"], pks=a["pks"], data=a["data"], ops=a["ops"]), a["host"], period=_period(pool, a["fmt"]), both=both)


def _junk_in_front(a, junk=7):
    """DER signatures packed behind `junk` bytes no offset points at: (data, offsets with offsets[0] == junk)"""
    from secp256k1_zkp_amd import Engine
    data, off = Engine.pack(a["sigs"])
    return np.concatenate([np.full(junk, 0x30, np.uint8), data]), (off + junk).astype(np.uint64)


def test_group_shares(groups, pool):
    """groups of three and of two engines: every share but the first starts at lo > 0, where the `_group` form adds 64 * lo (or hands
    on sig_off + lo), 32 * lo, pkb * lo (33, 64, 65) and ob * lo (33, 64) to the caller's arrays, in both of its branches.  Every
    combination of signature, key and opening format at 599 items (share starts 199 and 399, and 299, or a few less where items have
    no object form: the pool's period divides none of them) and at 4; the default one also at 1 .. 5 (empty shares), 65 and 257.
    DER: once more with the packed array behind 7 bytes of junk, so that no share's window starts where its offsets say before they
    are rebased.  The verdicts are the pool's."""
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for fmt in S.FORMAT_COMBINATIONS:
        for n in GROUP_SIZES if fmt == (0, 0, 0) else (599, 4):
            a = _arrays(_take(pool, n, start=5), *fmt)
            m = a["n"]
            assert m == n if fmt == (0, 0, 0) else m >= (540 if n == 599 else n - 1)      # (an item whose flipped bit broke a parser has no object form)
            for g in groups:
                _split_ok((fmt, n, len(g)), pool, a, E.share_starts(m, len(g)), both=m >= 257)
                got = _host(g, a)
                assert np.array_equal(got, a["host"]), (fmt, n, len(g), np.flatnonzero(got != a["host"])[:8], _names(a, got, a["host"])[:4])
                if fmt[1] == 0:
                    got = _commit(g, a)
                    assert np.array_equal(got, a["commit"]), (fmt, n, len(g), np.flatnonzero(got != a["commit"])[:8], _names(a, got, a["commit"])[:4])
            if fmt[0] == 2 and n == 599:
                g = groups[0]; L = g._lib
                data, off = _junk_in_front(a)
                assert off[0] == 7 and off[-1] == data.size
                res = np.full(m, 7, np.int32)
                assert L.secp256k1_anti_exfil_host_verify_batch_group(g._h, p(res), p(data), p(off), 2, p(a["msgs"]), p(a["pks"]), fmt[1], p(a["data"]), p(a["ops"]), fmt[2], m) == 1
                assert np.array_equal(res, a["host"]), (fmt, "junk in front", np.flatnonzero(res != a["host"])[:8])
                res[:] = 7
                assert L.secp256k1_ecdsa_s2c_verify_commit_batch_group(g._h, p(res), p(data), p(off), 2, p(a["data"]), p(a["ops"]), fmt[2], m) == 1
                assert np.array_equal(res, a["commit"]), (fmt, "junk in front", np.flatnonzero(res != a["commit"])[:8])


def test_group_argument_checks(groups, pool):
    """a NULL array or a format out of range through both `_group` forms: 0 with the argument status, and nothing marked valid"""
    g = groups[0]; L = g._lib; h = g._h
    a = _arrays(_take(pool, 6), 0, 0, 0)
    res = np.full(6, 7, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(a["sigs"]), None, 0, p(a["data"]), p(a["ops"]), 0, 6]
    assert L.secp256k1_ecdsa_s2c_verify_commit_batch_group(h, *good) == 1 and np.array_equal(res, a["commit"])
    for k, bad in ((0, None), (1, None), (4, None), (5, None), (3, 3), (3, -1), (6, 2), (6, -1), (3, 2)):      # (sig_format 2 without offsets: a NULL array)
        b = list(good); b[k] = bad; res[:] = 7
        assert L.secp256k1_ecdsa_s2c_verify_commit_batch_group(h, *b) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), (k, bad)
    good = [p(res), p(a["sigs"]), None, 0, p(a["msgs"]), p(a["pks"]), 0, p(a["data"]), p(a["ops"]), 0, 6]
    assert L.secp256k1_anti_exfil_host_verify_batch_group(h, *good) == 1 and np.array_equal(res, a["host"])
    for k, bad in ((0, None), (1, None), (4, None), (5, None), (7, None), (8, None), (3, 3), (3, -1), (6, 3), (6, -1), (9, 2), (9, -1), (3, 2)):
        b = list(good); b[k] = bad; res[:] = 7
        assert L.secp256k1_anti_exfil_host_verify_batch_group(h, *b) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), (k, bad)
    assert L.secp256k1_ecdsa_s2c_verify_commit_batch_group(h, None, None, None, 0, None, None, 0, 0) == 1
    assert L.secp256k1_anti_exfil_host_verify_batch_group(h, None, None, None, 0, None, None, 0, None, None, 0, 0) == 1


@pytest.mark.parametrize("fused", (0, 1))
def test_sub_range_launches_other_widths(pool, fused):
    """700 items (less the few without an object form) on an engine whose launches take 256 and then 512 lanes, in the default form and
    with S2K_OPT_S2C_FUSED: object signatures, DER signatures next to 65-byte keys (every launch reads its own window of the offsets),
    keys of 64 and 65 bytes, openings of 64.  Host and _dev form of both verifiers, against the pool's verdicts."""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_S2C_FUSED, fused)
        for fmt in SPLIT_FORMATS:
            a = _arrays(_take(pool, 700, start=3), *fmt)
            assert a["n"] >= 640 and 0 < a["host"].sum() < a["commit"].sum() < a["n"]
            for lanes in (256, 512):
                _split_ok((fmt, lanes, fused), pool, a, E.launch_starts(a["n"], lanes))
                eng.set_option(Engine.OPT_MAX_LANES, lanes)
                got = _host(eng, a)
                assert np.array_equal(got, a["host"]), (fmt, lanes, fused, _names(a, got, a["host"])[:4])
                got = _commit(eng, a)
                assert np.array_equal(got, a["commit"]), (fmt, lanes, fused, _names(a, got, a["commit"])[:4])
                d_c, d_h = _both_dev(eng, a)
                eng.sync()
                assert np.array_equal(d_c.cpu().numpy(), a["commit"]) and np.array_equal(d_h.cpu().numpy(), a["host"]), (fmt, lanes, fused, "dev")
    finally:
        eng.set_option(Engine.OPT_S2C_FUSED, 0)
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_host_commit_sub_range_launches():
    """600 different rand32 on an engine whose launches take 256 lanes (launch i0 reads rand32 + 32 * i0 and writes the commitments at
    32 * i0; the last launch is partial), host and _dev form, against the Python model's commitments"""
    import torch
    from secp256k1_zkp_amd import Engine
    rnd = np.random.default_rng(5612).integers(0, 256, (600, 32), dtype=np.uint8)
    want = np.frombuffer(b"".join(S.host_commit(rnd[i].tobytes()) for i in range(600)), np.uint8).reshape(600, 32)
    assert S.host_commit(bytes(32)) == hashlib.sha256(hashlib.sha256(S.TAG_DATA).digest() * 2 + bytes(32)).digest()
    E.check("host commit", E.launch_starts(600, 256), dict(rnd=rnd), np.ones(600, np.int32), both=False)
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        got = eng.anti_exfil_host_commit_batch(rnd)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
        d_out = torch.full((600, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
        eng.anti_exfil_host_commit_batch_dev(d_out, _dev(rnd))
        eng.sync()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()
