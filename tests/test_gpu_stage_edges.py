"""GPU tier of the host stager (csrc/engine_lanes.h) in the families that have a workspace beside their staged buffers: what it decides
is which buffers are skipped (nothing to upload) or handed on as NULL (an optional array the caller left out).  Each case goes through
the HOST form with the caller's pointer really NULL, and is held against the reference the family's own file uses: the reference's
multi-scalar multiplication, its recorded half-aggregates (tests/halfagg_batch_cases.py), the per-item verifiers and the hashlib seeds.
(s2k_ecmult_multi_many with either optional array left out, secp256k1_schnorrsig_aggverify_amd with n = 0 and the two verify_all forms
with and without results and seed are also reached by their families' files, at other sizes.)"""
import numpy as np
import pytest

from tests import bppp_all_cases as BC
from tests import bppp_all_ref as BR
from tests import halfagg_batch_cases as H
from tests import schnorr_all_cases as SC
from tests import schnorr_all_ref as SR
from tests.test_gpu_msm import _points
from tests.test_gpu_msm_many import _check_many

pytestmark = pytest.mark.gpu


def _three_sums(engine):
    """K = 3 sums of 0, 1 and 2 terms"""
    rng = np.random.default_rng(2024)
    off = np.array([0, 0, 1, 3], np.uint64)
    return rng, off, rng.integers(0, 256, (3, 32), dtype=np.uint8), _points(engine, rng, 3), rng.integers(0, 256, (3, 32), dtype=np.uint8), np.array([0, 1, 0], np.uint8)


def test_many_sums_without_pt_inf_without_g_sc_and_with_both(engine, ref):
    rng, off, sc, pts, g, inf = _three_sums(engine)
    _check_many(engine, ref, sc, pts, off, g, None)
    _check_many(engine, ref, sc, pts, off, None, inf)
    _check_many(engine, ref, sc, pts, off, g, inf)


def _small():
    by = {c.name: c for c in H.cases()}
    batch = [by["n=0"], by["n=1"], by["n=2"]]
    assert [c.n for c in batch] == [0, 1, 2] and all(c.sigs is not None and c.result == 1 for c in batch)
    return batch


def test_aggregates_of_0_1_and_2_items(engine):
    """the plain aggregation; the incremental one with nothing new (new_sigs64 NULL) and with nothing old"""
    batch = _small()
    keys, msgs, want = [c.keys[0] for c in batch], [c.msgs for c in batch], [c.agg for c in batch]
    res, aggs = engine.schnorrsig_aggregate_batch(keys, msgs, [c.sigs for c in batch])
    assert res.tolist() == [1, 1, 1] and aggs == want
    res, aggs = engine.schnorrsig_inc_aggregate_batch(want, keys, msgs, [b"", b"", b""])
    assert res.tolist() == [1, 1, 1] and aggs == want
    res, aggs = engine.schnorrsig_inc_aggregate_batch([b"\xff" * 32] * 3, keys, msgs, [c.sigs for c in batch])      # (n_before = 0: s_old is never read)
    assert res.tolist() == [1, 1, 1] and aggs == want


def test_aggverify_with_no_item_at_all(engine):
    """two empty aggregates in one batch (no key, no message: both arrays NULL), and the single-aggregate call with n = 0"""
    empty = _small()[0]
    assert engine.schnorrsig_aggverify_batch([b"", b""], [b"", b""], [empty.agg, empty.agg]).tolist() == [empty.result] * 2
    assert engine.schnorrsig_aggverify(b"", b"", empty.agg, n=0) == empty.result


def test_schnorr_verify_all_of_two_with_and_without_results_and_seed(engine, ref):
    import torch
    s, m, k = (x.copy() for x in SC.valid_batch(ref, 2))
    s[1, 40] ^= 4
    assert engine.schnorrsig_verify_batch(s, m, k).tolist() == [1, 0]
    v, res, seed = engine.schnorrsig_verify_all(s, m, k, locate=True, want_seed=True)
    assert v == 0 and res.tolist() == [1, 0] and seed == SR.seed(s, m, k, 32, 0)
    assert engine.schnorrsig_verify_all(s, m, k) == 0                                           # results and seed32_out NULL
    d_s, d_m, d_k = (torch.from_numpy(x).to("cuda:0") for x in (s, m, k))
    d_v = torch.full((1,), -7, dtype=torch.int32, device="cuda:0"); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.schnorrsig_verify_all_dev(d_v, d_s, d_m, d_k, seed_out=d_seed)
    engine.sync()
    assert int(d_v.cpu()[0]) == 0 and d_seed.cpu().numpy().tobytes() == seed


def test_bppp_verify_all_of_two_with_and_without_results_and_seed(engine, ref):
    import torch
    b = BC.copy(BC.valid_batch(ref, (4, 4), 2))
    b[0][1, 40] ^= 4
    proofs, trs, rhos, gens, g_len, cvs, commits = b
    assert engine.bppp_norm_product_verify_batch(*b).tolist() == [1, 0]
    v, res, seed = engine.bppp_norm_product_verify_all(*b, locate=True, want_seed=True)
    assert v == 0 and res.tolist() == [1, 0] and seed == BR.seed(*b)
    assert engine.bppp_norm_product_verify_all(*b) == 0                                         # results and seed32_out NULL
    d_p, d_t, d_r, d_g, d_c, d_m = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (proofs, trs, rhos, gens, cvs, commits))
    d_v = torch.full((1,), -7, dtype=torch.int32, device="cuda:0"); d_seed = torch.full((32,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.bppp_norm_product_verify_all_dev(d_v, d_p, proofs.shape[1], d_t, d_r, d_g, gens, g_len, d_c, cvs.shape[1], d_m, 2, seed_out=d_seed)
    engine.sync()
    assert int(d_v.cpu()[0]) == 0 and d_seed.cpu().numpy().tobytes() == seed


def test_a_refusal_behind_the_uploads_leaves_the_engine_usable(engine, ref):
    """S2K_OPT_MSM_MAX_TERMS lowered under a sum that is above the many-sums limit: the device part refuses the call after its inputs were
    staged (an ordinary error return); the next call of the same engine is served"""
    from secp256k1_zkp_amd import Engine, S2KError, _native
    n = H.MM_MAX_TERMS + 1
    sc = np.zeros((n, 32), np.uint8); pts = np.zeros((n, 64), np.uint8)                         # (never looked at: the first sum is the refused one)
    engine.set_option(Engine.OPT_MSM_MAX_TERMS, H.MM_MAX_TERMS)
    try:
        with pytest.raises(S2KError):
            engine.ecmult_multi_many(sc, pts, np.array([0, n], np.uint64))
        assert "exceeds what one launch indexes" in _native.last_error()
    finally:
        engine.set_option(Engine.OPT_MSM_MAX_TERMS, 0)
    rng, off, sc, pts, g, inf = _three_sums(engine)
    _check_many(engine, ref, sc, pts, off, g, inf)
