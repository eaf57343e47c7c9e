"""GPU parity of the batch half-aggregate calls, through the C ABI in the host and the `_dev` forms: the reference's recorded aggregates
and verdicts (tests/golden/halfagg_batch_vectors.json) in the batch shapes of the CPU tier (tests/halfagg_batch_cases.py), the
aggregator feeding the verifier on the device without a copy back, an aggregate above the many-sums limit between two small ones, and
a batch of one against the single-aggregate call.  Reads only the committed fixture and the engine."""
import ctypes

import numpy as np
import pytest

from tests import halfagg_batch_cases as H

pytestmark = pytest.mark.gpu


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dev(a):
    import torch
    t = torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to("cuda:0")
    torch.cuda.synchronize()          # (the calls below run on the engine's own stream)
    return t


def _dp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _filled(n, dtype=None):
    import torch
    t = torch.full((max(n, 1),), 0x6E, dtype=dtype or torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _ok(engine, r, what):
    from secp256k1_zkp_amd import _native
    assert r == 1, (what, _native.last_error())


def _verify(engine, dev):
    L, h = engine._lib, engine._h

    def host(keys, pk_format, msgs, item_off, aggs, agg_off):
        n = item_off.size - 1; res = np.full(n, -7, np.int32)
        _ok(engine, L.secp256k1_schnorrsig_aggverify_batch(h, _p(res), _p(keys), pk_format, _p(msgs), _p(item_off), _p(aggs), _p(agg_off), n), "aggverify_batch")
        return res

    def device(keys, pk_format, msgs, item_off, aggs, agg_off):
        import torch
        n = item_off.size - 1; d_res = _filled(n, torch.int32)
        d_k, d_m, d_a = _dev(keys), _dev(msgs), _dev(aggs)
        _ok(engine, L.secp256k1_schnorrsig_aggverify_batch_dev(h, None, _dp(d_res), _dp(d_k), pk_format, _dp(d_m), _p(item_off), _dp(d_a), _p(agg_off), n), "aggverify_batch_dev")
        engine.sync()
        return d_res.cpu().numpy()[:n]
    return device if dev else host


def _inc(engine, dev):
    L, h = engine._lib, engine._h

    def host(old, nb, keys, pk_format, msgs, new, item_off):
        n = item_off.size - 1; res = np.full(n, -7, np.int32); out = np.full(32 * (int(item_off[-1]) + n), 0xEE, np.uint8)
        if old is None:
            _ok(engine, L.secp256k1_schnorrsig_aggregate_batch(h, _p(res), _p(out), _p(keys), pk_format, _p(msgs), _p(new), _p(item_off), n), "aggregate_batch")
        else:
            _ok(engine, L.secp256k1_schnorrsig_inc_aggregate_batch(h, _p(res), _p(out), _p(old), _p(nb), _p(keys), pk_format, _p(msgs), _p(new), _p(item_off), n), "inc_aggregate_batch")
        return res, out.tobytes()

    def device(old, nb, keys, pk_format, msgs, new, item_off):
        import torch
        n = item_off.size - 1; ob = 32 * (int(item_off[-1]) + n)
        d_res, d_out = _filled(n, torch.int32), _filled(ob)
        d_k, d_m, d_s = _dev(keys), _dev(msgs), _dev(new)
        if old is None:
            _ok(engine, L.secp256k1_schnorrsig_aggregate_batch_dev(h, None, _dp(d_res), _dp(d_out), _dp(d_k), pk_format, _dp(d_m), _dp(d_s), _p(item_off), n), "aggregate_batch_dev")
        else:
            d_o = _dev(old)
            _ok(engine, L.secp256k1_schnorrsig_inc_aggregate_batch_dev(h, None, _dp(d_res), _dp(d_out), _dp(d_o), _p(nb), _dp(d_k), pk_format, _dp(d_m), _dp(d_s), _p(item_off), n),
                "inc_aggregate_batch_dev")
        engine.sync()
        return d_res.cpu().numpy()[:n], d_out.cpu().numpy()[:ob].tobytes()
    return device if dev else host


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("pk_format", [0, 1])
def test_every_vector_alone(engine, pk_format, dev):
    for c in H.cases():
        H.check_verify(_verify(engine, dev), [c], pk_format)


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("pk_format", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_batches_at_a_wavefront_edge(engine, m, pk_format, dev):
    H.check_verify(_verify(engine, dev), H.of_count(m), pk_format)


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("pk_format", [0, 1])
@pytest.mark.parametrize("m", [63, 64, 65, 130])
def test_exactly_m_chain_lanes(engine, m, pk_format, dev):
    """every aggregate owns a lane of k_hab_chain (n >= 1, right length, mixed sizes): 63 lanes, a full wavefront, a second workgroup with
    one lane, and three workgroups -- in the verifier and in the aggregator"""
    batch = H.with_lanes(m)
    assert all(H.owns_lane(c) for c in batch) and len(batch) == m
    H.check_verify(_verify(engine, dev), batch, pk_format)
    H.check_aggregate(_inc(engine, dev), H.good_with_lanes(m), pk_format)


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("pk_format", [0, 1])
def test_shuffled_batch(engine, pk_format, dev):
    H.check_verify(_verify(engine, dev), H.shuffled(), pk_format)


@pytest.mark.parametrize("dev", [0, 1])
def test_over_the_limit_between_two_small_ones(engine, dev):
    """4 097 signatures: 8 194 terms, above the many-sums limit of 8 192 -- the single-aggregate path inside the batch call"""
    by = {c.name: c for c in H.cases()}
    big = H.repeated()
    assert 2 * big.n > H.MM_MAX_TERMS >= 2 * (big.n - 1)
    H.check_verify(_verify(engine, dev), [by["n=2"], big, by["n=2 s off by one"]], 0)
    spoiled = H.Case("repeated, s off by one", big.n, big.keys[0], big.keys[1], big.msgs, big.agg[:-1] + bytes([big.agg[-1] ^ 1]), 0)
    H.check_verify(_verify(engine, dev), [by["n=2"], spoiled, by["n=3"]], 0)


@pytest.mark.parametrize("dev", [0, 1])
@pytest.mark.parametrize("pk_format", [0, 1])
def test_aggregation_against_the_reference(engine, pk_format, dev):
    good = H.good()
    H.check_aggregate(_inc(engine, dev), good, pk_format)
    H.check_aggregate(_inc(engine, dev), [good[i] for i in (7, 0, 3, 1, 6, 2, 5, 4)], pk_format)
    H.check_aggregate_refusals(_inc(engine, dev), pk_format)


def test_aggregate_of_the_repeated_triple(engine):
    big = H.repeated()
    keys, msgs, item_off = H._u8(big.keys[0]), H._u8(big.msgs), H.offsets([big.n])
    res, out = _inc(engine, 1)(None, None, keys, 0, msgs, H._u8(big.sigs), item_off)
    assert int(res[0]) == 1 and out == big.agg


def test_aggregate_then_verify_on_the_device(engine):
    """aggregate_batch_dev -> aggverify_batch_dev with aggsig_off[k] = 32 (item_off[k] + k), nothing copied back in between"""
    import torch
    L, h = engine._lib, engine._h
    batch = H.good_with_lanes(150) + [H.good()[0]] * 3         # 150 chain lanes (three workgroups of the chain kernel) and three empty aggregates
    assert H.good()[0].n == 0
    n = len(batch)
    item_off = H.offsets([c.n for c in batch]); agg_off = np.array([32 * (int(item_off[k]) + k) for k in range(n + 1)], np.uint64)
    d_k, d_m, d_s = _dev(H._u8(b"".join(c.keys[0] for c in batch))), _dev(H._u8(b"".join(c.msgs for c in batch))), _dev(H._u8(b"".join(c.sigs for c in batch)))
    d_made, d_verdict, d_out = _filled(n, torch.int32), _filled(n, torch.int32), _filled(int(agg_off[-1]))
    _ok(engine, L.secp256k1_schnorrsig_aggregate_batch_dev(h, None, _dp(d_made), _dp(d_out), _dp(d_k), 0, _dp(d_m), _dp(d_s), _p(item_off), n), "aggregate_batch_dev")
    _ok(engine, L.secp256k1_schnorrsig_aggverify_batch_dev(h, None, _dp(d_verdict), _dp(d_k), 0, _dp(d_m), _p(item_off), _dp(d_out), _p(agg_off), n), "aggverify_batch_dev")
    engine.sync()
    assert d_made.cpu().tolist() == [1] * n and d_verdict.cpu().tolist() == [1] * n
    assert H.out_slices(item_off, d_out.cpu().numpy().tobytes()) == [c.agg for c in batch]


@pytest.mark.parametrize("pk_format", [0, 1])
def test_batch_of_one_equals_the_single_call(engine, pk_format):
    for c in H.cases():
        keys, msgs, item_off, aggs, agg_off, want = H.pack_verify([c], pk_format)
        got = int(_verify(engine, 0)(keys, pk_format, msgs, item_off, aggs, agg_off)[0])
        single = engine.schnorrsig_aggverify(c.keys[pk_format], c.msgs, c.agg, pk_format=pk_format, n=c.n)
        assert got == single == want[0], c.name


def test_python_methods(engine):
    good = H.good()
    res, aggs = engine.schnorrsig_aggregate_batch([c.keys[0] for c in good], [c.msgs for c in good], [c.sigs for c in good])
    assert res.tolist() == [1] * len(good) and aggs == [c.agg for c in good]
    cs = H.shuffled()
    assert engine.schnorrsig_aggverify_batch([c.keys[1] for c in cs], [c.msgs for c in cs], [c.agg for c in cs], pk_format=1).tolist() == [c.result for c in cs]
    two = [c for c in good if c.n >= 2]
    # the first signature's own s is its one-signature aggregate's s (z_0 = 1)
    res, aggs3 = engine.schnorrsig_inc_aggregate_batch([c.sigs[:64] for c in two], [c.keys[0] for c in two], [c.msgs for c in two], [c.sigs[64:] for c in two])
    assert res.tolist() == [1] * len(two) and aggs3 == [c.agg for c in two]
