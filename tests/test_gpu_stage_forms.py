"""GPU tier of the forms that were the last to be staged by hand and now go through the host stager (csrc/engine_lanes.h):
s2k_ecmult_multi and its group form, rangeproof rewind, surjection proofs and Pedersen tallies -- at their optional arrays (the caller's
pointer really NULL), empty shares and second launches -- and the stager's own ordering of its uploads behind work that another stream
still has in flight.  Every expectation comes from the reference (tests/refapi.py) or from what the family's own file uses; the other
staged families are in tests/test_gpu_stage_edges.py."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_group import group2  # noqa: F401  (the two-engine group fixture)
from tests.test_gpu_msm import _points

pytestmark = pytest.mark.gpu


# ---- s2k_ecmult_multi, host form -------------------------------------------------------------------------------------------------
def _msm_inputs(engine, seed, n):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8); pts = _points(engine, rng, max(n, 1))[:n]
    inf = np.zeros(n, np.uint8); inf[1:2] = 1
    return sc, pts, inf, bytes(rng.integers(0, 256, 32, dtype=np.uint8))


def _check_msm(eng, ref, sc, pts, g, inf):
    want, winf = ref.ecmult_multi(sc, pts, g, inf)
    got, ginf = eng.ecmult_multi(sc, pts, g, inf)
    assert ginf == winf and (winf or got.tobytes() == want.tobytes()), (sc.shape[0], g is not None, inf is not None)


def test_msm_host_form_with_each_optional_array_left_out(engine, ref):
    sc, pts, inf, g = _msm_inputs(engine, 3101, 3)
    _check_msm(engine, ref, sc[:0], pts[:0], g, None)              # n = 0: the generator term alone
    _check_msm(engine, ref, sc, pts, None, inf)                    # g_sc NULL
    _check_msm(engine, ref, sc, pts, g, None)                      # pt_inf NULL
    _check_msm(engine, ref, sc, pts, g, inf)


def test_msm_host_form_above_the_launch_limit(engine, ref):
    """S2K_OPT_MSM_MAX_TERMS at its smallest value and 2 * cap + 3 terms: three launches whose scratch lies behind the staged inputs"""
    from secp256k1_zkp_amd import Engine
    cap = 64
    sc, pts, inf, g = _msm_inputs(engine, 3102, 2 * cap + 3)
    engine.set_option(Engine.OPT_MSM_MAX_TERMS, cap)
    try:
        _check_msm(engine, ref, sc, pts, g, inf)
        _check_msm(engine, ref, sc, pts, None, None)
    finally:
        engine.set_option(Engine.OPT_MSM_MAX_TERMS, 0)


# ---- the group's term-sharded sum, host form -----------------------------------------------------------------------------------------
def test_group_msm_with_empty_shares(group2, engine, ref):
    sc, pts, inf, g = _msm_inputs(engine, 3103, 1)
    _check_msm(group2, ref, sc[:0], pts[:0], g, None)              # n = 0: both shares empty, the generator term rides with engine 0
    _check_msm(group2, ref, sc, pts, g, None)                      # n = 1: one engine has an empty share and no generator term
    _check_msm(group2, ref, sc, pts, None, None)


def test_group_msm_with_slices_above_the_launch_limit(group2, engine, ref):
    """every engine's slice is 2 * cap + 3 terms: its staged slice lies behind the workspace of a sum that runs in pieces"""
    from secp256k1_zkp_amd import Engine
    cap = 64
    sc, pts, inf, g = _msm_inputs(engine, 3104, 2 * (2 * cap + 3))
    members = [group2.engine(i) for i in range(len(group2))]
    for m in members: m.set_option(Engine.OPT_MSM_MAX_TERMS, cap)
    try:
        _check_msm(group2, ref, sc, pts, g, inf)
        _check_msm(group2, ref, sc, pts, None, None)
    finally:
        for m in members: m.set_option(Engine.OPT_MSM_MAX_TERMS, 0)


# ---- rangeproof rewind, host form ---------------------------------------------------------------------------------------------------
def _ref_rewind(ref, commits, plist, gens, nonces, cap, extra):
    """secp256k1_rangeproof_rewind of the reference library per item, with the item's extra_commit: (results, blinds, values, messages)"""
    L = ref.lib
    vp, buf = ctypes.c_void_p, lambda a: np.ascontiguousarray(a, np.uint8).ctypes.data_as(ctypes.c_void_p)
    L.secp256k1_context_create.restype = vp
    ctx = vp(L.secp256k1_context_create(1))                                                  # SECP256K1_CONTEXT_NONE
    res, blinds, vals, msgs = [], [], [], []
    for i, proof in enumerate(plist):
        c = ctypes.create_string_buffer(64); g = ctypes.create_string_buffer(gens[i].tobytes(), 64)
        assert L.secp256k1_pedersen_commitment_parse(ctx, c, buf(commits[i])) == 1
        blind = np.zeros(32, np.uint8); val, mn, mx = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        msg = np.zeros(max(cap, 1), np.uint8); ol = ctypes.c_size_t(cap)
        ex = extra[i] if extra is not None else b""
        r = L.secp256k1_rangeproof_rewind(ctx, buf(blind), ctypes.byref(val), buf(msg) if cap else None, ctypes.byref(ol) if cap else None, buf(nonces[i]), ctypes.byref(mn),
                                          ctypes.byref(mx), c, proof, ctypes.c_size_t(len(proof)), ex if ex else None, ctypes.c_size_t(len(ex)), g)
        res.append(r); blinds.append(blind); vals.append(val.value); msgs.append(msg[:ol.value].tobytes() if (r and cap) else b"")
    L.secp256k1_context_destroy(ctx)
    return np.array(res, np.int32), np.stack(blinds), np.array(vals, np.uint64), msgs


@pytest.mark.parametrize("cap", [0, 96])                                 # message_out NULL (outlen comes from the scratch) / given with outlen
def test_rewind_of_two_proofs_with_and_without_messages_and_extra(engine, ref, cap):
    rng = np.random.default_rng(3105)
    commits, plist, gens, values, blinds, nonces, _ = ref.make_rangeproofs_msg(2, rng, msg_len=40, min_bits=16)
    extra = [b"stage", b""]
    ecommits, eplist, egens = ref.make_rangeproofs_extra(2, rng, extra, min_bits=16)
    enonces = np.ascontiguousarray(ecommits[:, :32])                    # (what the reference-side maker signs these with)
    for c, p, g, nn, ex in ((commits, plist, gens, nonces, None), (ecommits, eplist, egens, enonces, extra)):
        want = _ref_rewind(ref, c, p, g, nn, cap, ex)
        assert want[0].tolist() == [1, 1]
        res, bl, val, msgs, mn, mx = engine.rangeproof_rewind_batch(c, p, g, nn, msg_capacity=cap, extra=ex)
        assert np.array_equal(res, want[0]) and np.array_equal(bl, want[1]) and np.array_equal(val, want[2]) and msgs == want[3]
    # extra left out (NULL) where the first proof was signed over some: what the reference says to that
    assert engine.rangeproof_rewind_batch(ecommits, eplist, egens, enonces, msg_capacity=cap)[0].tolist() == _ref_rewind(ref, ecommits, eplist, egens, enonces, cap, None)[0].tolist()


# ---- surjection proofs --------------------------------------------------------------------------------------------------------------
def _sj_dev(eng, proofs, tags, outs):
    import torch
    data, off = eng.pack(list(proofs))
    toff = np.concatenate([[0], np.cumsum([t.shape[0] for t in tags])]).astype(np.uint64)
    flat = np.concatenate([t.reshape(-1) for t in tags] + [np.zeros(64, np.uint8)])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_res = torch.full((len(proofs),), 7, dtype=torch.int32, device="cuda:0")
    d_pr, d_po, d_tg, d_to, d_out = d(np.concatenate([data, np.zeros(64, np.uint8)])), d(off), d(flat), d(toff), d(np.stack(outs))
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert eng._lib.secp256k1_surjectionproof_verify_batch_dev(eng._h, None, p(d_res), p(d_pr), p(d_po), p(d_tg), p(d_to), p(d_out), len(proofs)) == 1
    eng.sync()
    return d_res.cpu().numpy()


def test_surjection_second_launch_starts_at_item_256(ref):
    """an engine of 256 lanes and 257 proofs of ragged tag counts: the second launch is item 256 alone, found through absolute offsets"""
    from secp256k1_zkp_amd import Engine
    rng = np.random.default_rng(3106)
    kinds = [ref.make_surjection(rng, k, min(k, 2)) for k in (1, 2, 3, 5)]
    bad = bytearray(kinds[2][0]); bad[-1] ^= 1
    kinds.append((bytes(bad), kinds[2][1], kinds[2][2]))
    verdict = [ref.surjection_verify(*k) for k in kinds]
    assert verdict == [1, 1, 1, 1, 0]
    pick = [int(x) for x in rng.integers(0, len(kinds), 257)]; pick[255], pick[256] = 4, 3      # (the last one valid, its neighbour not)
    proofs, tags, outs = ([kinds[k][j] for k in pick] for j in range(3))
    want = np.array([verdict[k] for k in pick], np.int32)
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        assert np.array_equal(eng.surjectionproof_verify_batch(proofs, tags, np.stack(outs)), want)
        assert np.array_equal(_sj_dev(eng, proofs, tags, outs), want)
    finally:
        eng.close()


def test_surjection_batch_without_any_input_tag(engine, ref):
    """proofs over zero inputs (the reference parses them and answers 0): tag_off is all zeros and nothing is uploaded for the tags"""
    rng = np.random.default_rng(3107)
    proofs = [b"\0\0" + bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)]
    tags = [np.zeros((0, 64), np.uint8)] * 3
    outs = [ref.make_surjection(rng, 1, 1)[2] for _ in range(3)]
    want = [ref.surjection_verify(p, t, o) for p, t, o in zip(proofs, tags, outs)]
    assert want == [0, 0, 0]
    assert engine.surjectionproof_verify_batch(proofs, tags, np.stack(outs)).tolist() == want
    assert _sj_dev(engine, proofs, tags, outs).tolist() == want


# ---- Pedersen tallies ---------------------------------------------------------------------------------------------------------------
def _tally_calls(engine, data, off, npos):
    """(host form, `_dev` form) through the C entries; data None: commits33 really NULL"""
    import torch
    L = engine._lib
    n = off.size - 1
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    res = np.full(n, 7, np.int32)
    assert L.secp256k1_pedersen_verify_tally_batch(engine._h, vp(res), None if data is None else vp(data), vp(off), vp(npos), n) == 1
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    d_c = None if data is None else torch.from_numpy(data.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert L.secp256k1_pedersen_verify_tally_batch_dev(engine._h, None, ctypes.c_void_p(d_res.data_ptr()), None if d_c is None else ctypes.c_void_p(d_c.data_ptr()),
                                                       vp(off), vp(npos), n) == 1
    engine.sync()
    return res, d_res.cpu().numpy()


def test_tallies_of_0_1_and_9_commitments(engine, ref):
    """nine is above the run length of a partial-sum round, so a second round runs; the lone commitment cannot balance"""
    rng = np.random.default_rng(3108)
    none = np.zeros((0, 33), np.uint8)
    lone = ref.make_balanced_tally(rng, 1, 1)[0]
    tallies = [(none, none), (lone, none), ref.make_balanced_tally(rng, 3, 6)]
    want = ref.pedersen_verify_tally_many(tallies)
    assert want.tolist() == [1, 0, 1]
    data = np.ascontiguousarray(np.concatenate([x for t in tallies for x in t]))
    off = np.array([0, 0, 1, 10], np.uint64); npos = np.array([0, 1, 3], np.uint64)
    host, dev = _tally_calls(engine, data, off, npos)
    assert np.array_equal(host, want) and np.array_equal(dev, want)


def test_tallies_all_empty_with_no_commitment_array(engine, ref):
    none = np.zeros((0, 33), np.uint8)
    want = ref.pedersen_verify_tally_many([(none, none)] * 2)
    host, dev = _tally_calls(engine, None, np.zeros(3, np.uint64), np.zeros(2, np.uint64))
    assert np.array_equal(host, want) and np.array_equal(dev, want)


# ---- the stager orders its own uploads ------------------------------------------------------------------------------------------------
def test_host_form_behind_a_sum_in_flight_on_another_stream(engine, ref):
    """s2k_ecmult_multi_dev of 2^16 terms queued on a caller's stream, then -- nothing synchronised -- the host form s2k_ecmult_batch, whose
    uploads land where the sum's workspace starts: the stager makes the engine's stream wait for the sum first.  Both against the reference."""
    import torch
    from tests.refapi import G_XY
    rng = np.random.default_rng(3109)
    n = 1 << 16
    pts = _points(engine, rng, n); sc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want_xy, want_inf = ref.ecmult_multi(sc, pts)
    m = 3000
    a = pts[:m]; na = rng.integers(0, 256, (m, 32), dtype=np.uint8); ng = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    want_b, want_binf = ref.ecmult_batch(a, na, ng=ng)
    d_sc, d_pt = torch.from_numpy(sc.reshape(-1)).to("cuda:0"), torch.from_numpy(pts.reshape(-1).copy()).to("cuda:0")
    r_xy = torch.zeros(64, dtype=torch.uint8, device="cuda:0"); r_inf = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    engine.ecmult_batch(a[:8], na[:8], ng=ng[:8])                      # (tables and workspace exist before the two calls meet)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    engine.ecmult_multi_dev(r_xy, r_inf, d_sc, d_pt, stream=ctypes.c_void_p(side.cuda_stream))
    got_b, got_binf = engine.ecmult_batch(a, na, ng=ng)
    torch.cuda.synchronize()
    assert int(r_inf.cpu()[0]) == want_inf and r_xy.cpu().numpy().tobytes() == want_xy.tobytes()
    assert np.array_equal(got_binf, np.asarray(want_binf).reshape(-1)) and np.array_equal(got_b, want_b)
