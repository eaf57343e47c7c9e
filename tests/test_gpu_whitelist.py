"""GPU tier: whitelist-signature verification (k_wl_keys, k_wl_ring) through the host, `_dev` and `_amd` entry points, every verdict
against the unmodified reference asked in the run (oracle/_ref through tests/whitelist_ref.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wref(ref):
    from tests.whitelist_ref import WhitelistRef
    return WhitelistRef()


@pytest.fixture(scope="module")
def edges(wref):
    from tests.whitelist_ref import edge_cases
    return edge_cases(wref, with_255=False)


@pytest.fixture(scope="module")
def threes(wref):
    """300 signatures over ONE 3-key list, every fourth one corrupted, with the reference's verdicts: made once for the module"""
    from tests.whitelist_ref import random_items
    items = random_items(wref, 300, 3305, lengths=(3,))
    assert len({x[1] for x in items}) == 1
    return items


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(engine, items):
    """a list per item (list_of = NULL)"""
    return engine.whitelist_verify_batch([x[0] for x in items], [x[1] for x in items], [x[2] for x in items], b"".join(x[3] for x in items))


def _host_shared(engine, items):
    """one list for the whole batch"""
    return engine.whitelist_verify_batch([x[0] for x in items], [items[0][1]], [items[0][2]], b"".join(x[3] for x in items), list_of=np.zeros(len(items), np.uint32))


def _device(engine, items):
    """the same through secp256k1_whitelist_verify_batch_dev: byte arrays on cuda:0, offset arrays on the host"""
    import torch
    from secp256k1_zkp_amd import Engine
    sigs, sig_off = Engine.pack([x[0] for x in items])
    on, list_off = Engine.pack([x[1] for x in items]); off, _ = Engine.pack([x[2] for x in items])
    res = torch.full((len(items),), 7, dtype=torch.int32, device="cuda:0")
    engine.whitelist_verify_batch_dev(res, _dev(sigs), sig_off, _dev(on), _dev(off), list_off // np.uint64(64),
                                      _dev(np.frombuffer(b"".join(x[3] for x in items), np.uint8)))
    torch.cuda.synchronize()
    return res.cpu().numpy()


def _expect(items):
    return np.array([x[-1] for x in items], np.int32)


def test_edge_list_host_and_dev(engine, edges):
    items = [c[1:] for c in edges]
    want = _expect(items)
    assert want.sum() == 13 and len(items) == 40
    got = _host(engine, items)
    assert got.tolist() == want.tolist(), [c[0] for c, g, w in zip(edges, got, want) if g != w]
    got = _device(engine, items)
    assert got.tolist() == want.tolist(), [c[0] for c, g, w in zip(edges, got, want) if g != w]


def test_edge_list_amd(engine, edges, wref):
    """secp256k1_whitelist_verify_amd takes the parsed object: every case whose bytes secp256k1_whitelist_signature_parse accepts goes
    through it; the others have no object to hand over and must be refused by the parser"""
    from secp256k1_zkp_amd import _native
    L = _native.load()
    called = 0
    for name, sig, on, off, sub, verdict in edges:
        obj = wref.parse(sig)
        if obj is None:
            assert verdict == 0, name
            continue
        called += 1
        assert L.secp256k1_whitelist_verify_amd(None, ctypes.byref(obj), on + bytes(64), off + bytes(64), len(on) // 64, sub) == verdict, name
        assert L.s2k_last_status() == 0, name
    # 40 cases; the parser refuses five: the n_keys byte one too small / too large, one byte short / long, length 0
    assert called == 35
    obj = wref.parse(edges[0][1])
    for args in ((None, None, edges[0][2], edges[0][3], 1, edges[0][4]), (None, ctypes.byref(obj), None, edges[0][3], 1, edges[0][4]),
                 (None, ctypes.byref(obj), edges[0][2], None, 1, edges[0][4]), (None, ctypes.byref(obj), edges[0][2], edges[0][3], 1, None)):
        assert L.secp256k1_whitelist_verify_amd(*args) == 0 and L.s2k_last_status() == 2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wavefront_and_block_edges(engine, threes, n):
    """partial wavefronts and blocks (the dead lanes take part in the shared inversion); one shared list and a list per item agree"""
    items = threes[:n]
    want = _expect(items)
    if n >= 4:
        assert 0 < want.sum() < n
    a = _host_shared(engine, items); b = _host(engine, items)
    assert a.tolist() == b.tolist() == want.tolist()
    assert _device(engine, items).tolist() == want.tolist()


def test_mixed_lengths_in_one_wavefront(engine, wref, edges):
    """list lengths 0, 1, 2 and 5, valid and invalid, interleaved in one wavefront: a lane that finishes its ring early rides along and
    must not change a neighbour's verdict"""
    from tests.whitelist_ref import random_items
    pool = random_items(wref, 40, 3306, lengths=(1, 2, 5), corrupt_every=3)
    empty = [c[1:] for c in edges if c[0].startswith("crafted n=0")]
    items = []
    for k in range(60):
        items.append(empty[(k // 4) % 2] if k % 4 == 0 else pool[(7 * k) % len(pool)])
    want = _expect(items)
    assert {len(x[1]) // 64 for x in items} == {0, 1, 2, 5} and 0 < want.sum() < len(items)
    assert _host(engine, items).tolist() == want.tolist()
    assert _device(engine, items).tolist() == want.tolist()


def test_sub_range_launches(engine, threes):
    """S2K_OPT_MAX_LANES = 256 with 300 items of 3 keys: 900 pairs are four launches of k_wl_keys, 300 items two of k_wl_ring"""
    from secp256k1_zkp_amd import Engine
    want = _expect(threes)
    base = _host_shared(engine, threes)
    assert base.tolist() == want.tolist()
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        assert _host_shared(eng, threes).tolist() == base.tolist()
        assert _host(eng, threes).tolist() == base.tolist()
        assert _device(eng, threes).tolist() == base.tolist()
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_255_keys(engine, wref):
    from tests.whitelist_ref import edge_cases
    big = [c for c in edge_cases(wref, with_255=True) if "255" in c[0]]
    assert [c[5] for c in big] == [1, 0] and len(big[0][2]) == 255 * 64
    items = [c[1:] for c in big]
    assert _host(engine, items).tolist() == [1, 0]
    assert _host_shared(engine, items).tolist() == [1, 0]


def test_junk_takes_no_work(engine, threes, wref):
    """every signature has the wrong length: all 0 (and no key lanes: the plan counts none)"""
    items = [(x[0][:-1] if k % 2 else x[0] + b"\0", x[1], x[2], x[3]) for k, x in enumerate(threes[:70])]
    for x in items[:4]:
        assert wref.verify(*x) == 0
    assert _host_shared(engine, items).tolist() == [0] * 70
    assert _device(engine, items).tolist() == [0] * 70


def test_argument_errors(engine, threes):
    """a list_of entry out of range and decreasing list_off: return 0, S2K_STATUS_ILLEGAL_ARGUMENT, results zeroed"""
    from secp256k1_zkp_amd import Engine
    L, h = engine._lib, engine._h
    items = threes[:4]
    sigs, sig_off = Engine.pack([x[0] for x in items])
    on = np.frombuffer(items[0][1], np.uint8); off = np.frombuffer(items[0][2], np.uint8)
    subs = np.frombuffer(b"".join(x[3] for x in items), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good_off = np.array([0, 3], np.uint64); good_of = np.zeros(4, np.uint32)
    res = np.full(4, 7, np.int32)
    assert L.secp256k1_whitelist_verify_batch(h, p(res), p(sigs), p(sig_off), p(on), p(off), p(good_off), 1, p(good_of), p(subs), 4) == 1
    assert res.tolist() == _expect(items).tolist()
    for list_off, n_lists, list_of in ((good_off, 1, np.array([0, 0, 1, 0], np.uint32)), (np.array([0, 3, 2], np.uint64), 2, good_of),
                                       (np.array([1, 3], np.uint64), 1, good_of), (good_off, 1, None)):
        res = np.full(4, 7, np.int32)
        assert L.secp256k1_whitelist_verify_batch(h, p(res), p(sigs), p(sig_off), p(on), p(off), p(list_off), n_lists, None if list_of is None else p(list_of), p(subs), 4) == 0
        assert L.s2k_last_status() == 2 and res.tolist() == [0] * 4
    import torch
    dres = torch.full((4,), 7, dtype=torch.int32, device="cuda:0")
    d = [_dev(sigs), _dev(on), _dev(off), _dev(subs)]
    bad_of = np.array([0, 0, 1, 0], np.uint32)
    assert L.secp256k1_whitelist_verify_batch_dev(h, None, ctypes.c_void_p(dres.data_ptr()), ctypes.c_void_p(d[0].data_ptr()), p(sig_off), ctypes.c_void_p(d[1].data_ptr()),
                                                  ctypes.c_void_p(d[2].data_ptr()), p(good_off), 1, p(bad_of), ctypes.c_void_p(d[3].data_ptr()), 4) == 0
    assert L.s2k_last_status() == 2
    engine.sync()
    assert dres.cpu().tolist() == [0] * 4
    assert L.secp256k1_whitelist_verify_batch(h, None, p(sigs), p(sig_off), p(on), p(off), p(good_off), 1, p(good_of), p(subs), 4) == 0 and L.s2k_last_status() == 2
