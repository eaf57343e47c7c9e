"""GPU: asset generators and explicit-amount commitments (csrc/generator.h, csrc/engine_generator.hip) against the unmodified reference
(oracle/_ref through tests/generator_ref.py): every verdict and every output is the reference's, asked in this run (where the verdict
is 0 the output is zero bytes, the engine's contract)."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OPS = ("parse", "serialize", "generate", "generate blinded", "commit", "commit null")
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def gref(ref):
    from tests.generator_ref import GeneratorRef
    return GeneratorRef()


def _split(items):
    """items -> {kind: [items]}: generate and commit split by whether they carry blinds (NULL or not holds for a whole batch)"""
    out = {k: [] for k in OPS}
    for it in items:
        op, _, args, _, _ = it
        if op == "generate":
            out["generate" if args[1] is None else "generate blinded"].append(it)
        elif op == "commit":
            out["commit null" if args[0] is None else "commit"].append(it)
        else:
            out[op].append(it)
    return out


@pytest.fixture(scope="module")
def pools(gref):
    """per kind: the edge list in front, then seeded random items (600 per entry point); built once and never changed"""
    from tests.generator_ref import edge_cases, random_items
    e = _split(edge_cases(gref)); r = _split(random_items(gref, 600, 5505))
    out = {k: e[k] + r[k] for k in OPS}
    for k in OPS:
        assert len(out[k]) >= 190, (k, len(out[k]))
        if k != "serialize":
            assert any(it[3] == 0 for it in out[k][:len(e[k])]) or k == "generate"
    return out


def _pick(pool, n):
    """n items: edge and random items mixed in (every other item walks the edge part of the pool, which sits in front)"""
    return [pool[(i // 2) % len(pool)] if i % 2 == 0 else pool[len(pool) - 1 - (i // 2) % len(pool)] for i in range(n)]


def _u8(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy()


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


def _run(engine, kind, items, dev):
    """-> (verdicts, outputs) of the engine, (expected verdicts, expected outputs); _dev forms write into tensors pre-filled with 7 / 0xFF"""
    import torch
    n = len(items)
    exp_v = np.array([it[3] for it in items], np.int32)
    ow = 64 if kind in ("parse", "generate", "generate blinded") else 33
    exp_o = _u8([it[4] for it in items], ow)
    d_res = torch.full((n,), 7, dtype=torch.int32, device="cuda:0") if dev else None
    d_out = torch.full((n, ow), 0xFF, dtype=torch.uint8, device="cuda:0") if dev else None
    if kind == "parse":
        a = _u8([it[2][0] for it in items], 33)
        if dev:
            engine.generator_parse_batch_dev(d_res, d_out, _dev(a))
        else:
            got = engine.generator_parse_batch(a)
    elif kind == "serialize":
        a = _u8([it[2][0] for it in items], 64)
        if dev:
            engine.generator_serialize_batch_dev(d_out, _dev(a)); d_res.fill_(1)
        else:
            got = (np.ones(n, np.int32), engine.generator_serialize_batch(a))
    elif kind in ("generate", "generate blinded"):
        keys = _u8([it[2][0] for it in items], 32)
        blinds = _u8([it[2][1] for it in items], 32) if kind == "generate blinded" else None
        if dev:
            engine.generator_generate_batch_dev(d_res, d_out, _dev(keys), _dev(blinds))
        else:
            got = engine.generator_generate_batch(keys, blinds)
    else:
        blinds = _u8([it[2][0] for it in items], 32) if kind == "commit" else None
        values = np.array([it[2][1] for it in items], np.uint64)
        gens = _u8([it[2][2] for it in items], 64)
        if dev:
            engine.pedersen_commit_batch_dev(d_res, d_out, _dev(values), _dev(gens), _dev(blinds))
        else:
            got = engine.pedersen_commit_batch(values, gens, blinds)
    if dev:
        engine.sync()
        got = (d_res.cpu().numpy(), d_out.cpu().numpy())
    return got, (exp_v, exp_o)


def _assert_same(items, got, exp, what):
    bad = [it[1] for it, g, e, go, eo in zip(items, got[0], exp[0], got[1], exp[1]) if g != e or not np.array_equal(go, eo)]
    assert not bad, (what, bad[:6])


@pytest.mark.parametrize("kind", OPS)
def test_batch_sizes_host_and_dev(engine, pools, kind):
    """every entry point, host and _dev form, at 1, 63, 64, 65 and 257 items: one live lane in a wavefront, a full wavefront, one lane into
    the next, a block boundary plus one; edge and random items mixed"""
    for n in SIZES:
        items = _pick(pools[kind], n)
        for dev in (False, True):
            got, exp = _run(engine, kind, items, dev)
            _assert_same(items, got, exp, (kind, n, dev))
    if kind != "serialize":
        items = _pick(pools[kind], 257)
        zeros = sum(1 for it in items if it[3] == 0)
        assert 0 < zeros < 257 or kind == "generate"


@pytest.mark.parametrize("kind", OPS)
def test_sub_range_launches(pools, kind):
    """600 items on an engine whose launches take 256 lanes: the sub-launch loop with a ragged tail"""
    from secp256k1_zkp_amd import Engine
    eng = Engine(0)
    try:
        eng.set_option(Engine.OPT_MAX_LANES, 256)
        items = _pick(pools[kind], 600)
        for dev in (False, True):
            got, exp = _run(eng, kind, items, dev)
            _assert_same(items, got, exp, (kind, dev))
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()


def test_fixture_through_the_gpu(engine):
    from tests.generator_ref import from_json
    items = from_json(json.load(open(os.path.join(HERE, "golden", "generator_vectors.json")))["vectors"])
    for kind, its in _split(items).items():
        assert its, kind
        got, exp = _run(engine, kind, its, False)
        _assert_same(its, got, exp, kind)


@pytest.mark.parametrize("kind", ("parse", "generate blinded", "commit"))
def test_refused_first_lane(engine, pools, kind):
    """a batch whose first lane is a refused item (bad prefix, blind >= n): its neighbours in the same wavefront are still right, and so
    are the neighbours of a refused lane in the middle and at the end of a wavefront"""
    pool = pools[kind]
    bad = [it for it in pool if it[3] == 0 and ("refused" in it[1] or "blind n" in it[1] or "blind 2^256-1" in it[1])]
    good = [it for it in pool if it[3] == 1]
    assert bad and len(good) >= 64
    for pos in (0, 31, 63):
        items = good[:64]; items[pos] = bad[0]
        for dev in (False, True):
            got, exp = _run(engine, kind, items, dev)
            assert got[0][pos] == 0 and not got[1][pos].any()
            _assert_same(items, got, exp, (kind, pos, dev))
    items = [bad[i % len(bad)] for i in range(64)] + good[:1]             # a whole wavefront of refused items, then one live lane
    got, exp = _run(engine, kind, items, True)
    _assert_same(items, got, exp, (kind, "dead wavefront"))


@pytest.mark.parametrize("kind", ("commit null", "commit"))
def test_malformed_object_stays_with_its_item(engine, pools, kind):
    """a zeroed generator object (what parse and generate write for a refused item) and one with y = 0, at lanes 0, 31 and 63 of a commit
    batch, with NULL blinds and with blinds: that item reads 0 and 33 zero bytes, its 63 neighbours are the reference's byte for byte"""
    pool = pools[kind]
    good = [it for it in pool if it[3] == 1]
    assert len(good) >= 64
    for obj in ("all-zero object", "object with y = 0"):
        bad = [it for it in pool if it[1].startswith(obj) and " value 0 " not in it[1]]
        assert len(bad) == 3 and all(it[3] == 0 for it in bad)
        for pos in (0, 31, 63):
            for b in bad:
                items = good[:64]; items[pos] = b
                for dev in (False, True):
                    got, exp = _run(engine, kind, items, dev)
                    assert got[0][pos] == 0 and not got[1][pos].any(), (obj, pos, dev, b[1])
                    assert got[0].sum() == 63
                    _assert_same(items, got, exp, (kind, obj, pos, dev))
        items = good[:64]
        for pos, b in zip((0, 31, 63), bad):                                 # all three lanes at once
            items[pos] = b
        got, exp = _run(engine, kind, items, True)
        assert got[0].sum() == 61
        _assert_same(items, got, exp, (kind, obj, "three lanes"))


def test_refused_generators_feed_commit_in_hbm(engine, pools, gref):
    """parse_batch_dev -> commit_batch_dev without leaving HBM, one wire generator refused: only that item's commitment fails"""
    import torch
    good = [it for it in pools["parse"] if it[3] == 1][:64]
    bad = next(it for it in pools["parse"] if "refused" in it[1])
    items = list(good); items[0] = bad; items[40] = bad
    d_gen = torch.full((64, 64), 0xFF, dtype=torch.uint8, device="cuda:0"); d_r = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    d_c = torch.full((64, 33), 0xFF, dtype=torch.uint8, device="cuda:0"); d_r2 = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    values = np.arange(1, 65, dtype=np.uint64)
    engine.generator_parse_batch_dev(d_r, d_gen, _dev(_u8([it[2][0] for it in items], 33)))
    engine.pedersen_commit_batch_dev(d_r2, d_c, _dev(values), d_gen, None)
    engine.sync()
    exp_v = np.array([it[3] for it in items], np.int32)
    assert np.array_equal(d_r.cpu().numpy(), exp_v) and np.array_equal(d_r2.cpu().numpy(), exp_v)
    ref_c = _u8([gref.commit(None, int(v), it[4])[1] if it[3] else bytes(33) for v, it in zip(values, items)], 33)
    assert np.array_equal(d_c.cpu().numpy(), ref_c) and not ref_c[0].any() and not ref_c[40].any() and ref_c[1].any()


def test_zero_blinds_equal_no_blinds(engine, pools):
    """blind 0 gives the unblinded generator; NULL blinds give the zero-blind commitment"""
    plain = pools["generate"][:8]
    keys = _u8([it[2][0] for it in plain], 32)
    got = engine.generator_generate_batch(keys, np.zeros((8, 32), np.uint8))
    assert got[0].all() and np.array_equal(got[1], _u8([it[4] for it in plain], 64))
    cn = [it for it in pools["commit null"] if it[3] == 1][:8]
    values = np.array([it[2][1] for it in cn], np.uint64); gens = _u8([it[2][2] for it in cn], 64)
    got = engine.pedersen_commit_batch(values, gens, np.zeros((8, 32), np.uint8))
    assert got[0].all() and np.array_equal(got[1], _u8([it[4] for it in cn], 33))


def test_pipeline_in_hbm(engine, gref):
    """32 tallies from wire bytes to verdict without leaving HBM: asset ids -> generator_generate_batch_dev; fee values ->
    pedersen_commit_batch_dev with NULL blinds; the fee commitments beside blinded commitments made by the reference ->
    secp256k1_pedersen_verify_tally_batch_dev.  Verdicts equal secp256k1_pedersen_verify_tally on the reference's own objects.  Half of
    the tallies balance, half are off by one unit of fee."""
    import torch
    from tests.generator_ref import N, b32
    rng = np.random.default_rng(5506)
    T = 32
    ids = rng.integers(0, 256, (T, 32), dtype=np.uint8)
    d_gen = torch.full((T, 64), 0xFF, dtype=torch.uint8, device="cuda:0"); d_res = torch.full((T,), 7, dtype=torch.int32, device="cuda:0")
    engine.generator_generate_batch_dev(d_res, d_gen, _dev(ids))
    # the reference's side: input = output + fee, blinds summing to zero on both sides
    ref_gens = [gref.generate(ids[t].tobytes())[1] for t in range(T)]
    fees = rng.integers(1, 1 << 40, T, dtype=np.uint64)
    claimed = fees + np.array([0 if t % 2 == 0 else 1 for t in range(T)], np.uint64)        # odd tallies: off by one unit of fee
    ref_in, ref_out, ref_fee = [], [], []
    for t in range(T):
        v_out = int(rng.integers(1, 1 << 50)); bl = int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist()), "big") % N
        ref_in.append(gref.commit_obj(b32(bl), v_out + int(fees[t]), ref_gens[t]))
        ref_out.append(gref.commit_obj(b32(bl), v_out, ref_gens[t]))
        ref_fee.append(gref.commit_obj(bytes(32), int(claimed[t]), ref_gens[t]))
        assert ref_in[-1] and ref_out[-1] and ref_fee[-1]
    expected = np.array([gref.verify_tally([ref_in[t]], [ref_out[t], ref_fee[t]]) for t in range(T)], np.int32)
    assert expected.tolist() == [1 if t % 2 == 0 else 0 for t in range(T)]
    # the engine's side: the fee commitments are made on the device from the device-made generators
    d_fee = torch.full((T, 33), 0xFF, dtype=torch.uint8, device="cuda:0"); d_res2 = torch.full((T,), 7, dtype=torch.int32, device="cuda:0")
    engine.pedersen_commit_batch_dev(d_res2, d_fee, _dev(claimed), d_gen, None)
    engine.sync()                                                                             # (the assembly below runs on torch's stream, not the engine's)
    d_all = torch.empty((T, 3, 33), dtype=torch.uint8, device="cuda:0")                       # per tally: input | output, fee
    d_all[:, 0] = _dev(_u8([o[:33] for o in ref_in], 33)); d_all[:, 1] = _dev(_u8([o[:33] for o in ref_out], 33)); d_all[:, 2] = d_fee
    d_all = d_all.contiguous()
    off = np.arange(T + 1, dtype=np.uint64) * 3; npos = np.ones(T, np.uint64)
    d_verdict = torch.full((T,), 7, dtype=torch.int32, device="cuda:0")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert engine._lib.secp256k1_pedersen_verify_tally_batch_dev(engine._h, None, ctypes.c_void_p(d_verdict.data_ptr()), ctypes.c_void_p(d_all.data_ptr()),
                                                                 p(off), p(npos), T) == 1
    engine.sync()
    assert d_res.cpu().numpy().all() and d_res2.cpu().numpy().all()
    assert np.array_equal(d_gen.cpu().numpy(), _u8(ref_gens, 64))
    assert np.array_equal(d_fee.cpu().numpy(), _u8([o[:33] for o in ref_fee], 33))
    assert np.array_equal(d_verdict.cpu().numpy(), expected)


def test_single_item_forms(engine, pools):
    """the three _amd forms: one valid and one invalid item each, verdict and status"""
    L = engine._lib
    for it in (next(x for x in pools["generate"] if x[3] == 1),):
        o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_generator_generate_amd(None, o, it[2][0]) == 1 and o.raw == it[4] and L.s2k_last_status() == 0
    assert L.secp256k1_generator_generate_amd(None, None, bytes(32)) == 0 and L.s2k_last_status() == 2       # its only invalid item: ARG_CHECK
    for v in (1, 0):
        it = next(x for x in pools["parse"] if x[3] == v)
        o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_generator_parse_amd(None, o, it[2][0]) == v and o.raw == it[4] and L.s2k_last_status() == 0, it[1]
        it = next(x for x in pools["commit"] if x[3] == v)
        o = ctypes.create_string_buffer(b"\xAA" * 64, 64)
        assert L.secp256k1_pedersen_commit_amd(None, o, it[2][0], it[2][1], it[2][2]) == v and L.s2k_last_status() == 0, it[1]
        assert o.raw == it[4] + bytes(31), it[1]
    o = ctypes.create_string_buffer(64)
    assert L.secp256k1_pedersen_commit_amd(None, o, None, 1, bytes(64)) == 0 and L.s2k_last_status() == 2


def test_batch_argument_checks(engine, pools):
    """NULL where the reference has ARG_CHECK fails the call with the argument status; NULL blinds are legal; n == 0 succeeds"""
    L = engine._lib; h = engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    res = np.full(4, 7, np.int32); o64 = np.full((4, 64), 0xFF, np.uint8); o33 = np.full((4, 33), 0xFF, np.uint8)
    keys = np.zeros((4, 32), np.uint8); in33 = np.zeros((4, 33), np.uint8); vals = np.ones(4, np.uint64)
    gens = _u8([pools["serialize"][0][2][0]] * 4, 64)
    calls = (("secp256k1_generator_generate_batch", [p(res), p(o64), p(keys), None, 4], (0, 1, 2)),
             ("secp256k1_generator_parse_batch", [p(res), p(o64), p(in33), 4], (0, 1, 2)),
             ("secp256k1_generator_serialize_batch", [p(o33), p(gens), 4], (0, 1)),
             ("secp256k1_pedersen_commit_batch", [p(res), p(o33), None, p(vals), p(gens), 4], (0, 1, 3, 4)))
    for name, good, nullable in calls:
        f = getattr(L, name); fd = getattr(L, name + "_dev")
        assert f(h, *good) == 1, name
        for k in nullable:
            a = list(good); a[k] = None
            assert f(h, *a) == 0 and L.s2k_last_status() == 2, (name, k)
            assert fd(h, None, *a) == 0 and L.s2k_last_status() == 2, (name, k)
        a = list(good); a[-1] = 0
        assert f(h, *a) == 1 and fd(h, None, *([None] * (len(good) - 1)), 0) == 1, name
    assert engine.generator_parse_batch(b"")[0].size == 0
