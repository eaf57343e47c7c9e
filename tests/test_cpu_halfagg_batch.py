"""CPU tier of the batch half-aggregate calls: csrc/halfagg_batch.h compiled for the host (tests/host_emul/halfagg_batch_emu.cpp), driven
in the order engine_halfagg_batch.hip launches its kernels -- the lane -> aggregate permutation of the chain kernel, the state-slot rule,
the binary search, the partition at the many-sums limit -- against the reference's recorded aggregates and verdicts
(tests/golden/halfagg_batch_vectors.json), bit for bit, in both key formats; the C ABI's argument checks, the Python argument checks
and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import halfagg_batch_cases as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH = ["secp256k1_schnorrsig_aggverify_batch", "secp256k1_schnorrsig_aggregate_batch", "secp256k1_schnorrsig_inc_aggregate_batch"]
SYMBOLS = BATCH + [s + "_dev" for s in BATCH]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_halfagg_batch_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_halfagg_batch_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    return ctypes.CDLL(path)


def _verify(emu, limit=H.MM_MAX_TERMS):
    def call(keys, pk_format, msgs, item_off, aggs, agg_off):
        n = item_off.size - 1; res = np.full(n, -7, np.int32)
        assert emu.emu_halfagg_verify_batch(_p(res), _p(keys), pk_format, _p(msgs), _p(item_off), _p(aggs), _p(agg_off), ctypes.c_size_t(n), ctypes.c_uint64(limit)) == 1
        return res
    return call


def _inc(emu):
    def call(old, nb, keys, pk_format, msgs, new, item_off):
        n = item_off.size - 1; res = np.full(n, -7, np.int32); out = np.full(32 * (int(item_off[-1]) + n), 0xEE, np.uint8)
        if old is None:
            assert emu.emu_halfagg_aggregate_batch(_p(res), _p(out), _p(keys), pk_format, _p(msgs), _p(new), _p(item_off), ctypes.c_size_t(n)) == 1
        else:
            assert emu.emu_halfagg_inc_aggregate_batch(_p(res), _p(out), _p(old), _p(nb), _p(keys), pk_format, _p(msgs), _p(new), _p(item_off), ctypes.c_size_t(n)) == 1
        return res, out.tobytes()
    return call


def test_fixture_shape():
    g = H.golden()
    assert g["sizes"] == [0, 1, 2, 3, 4, 5, 16, 40] and g["repeated"]["count"] == 4097
    for rec in g["aggregates"]:
        names = [t["name"] for t in rec["tampered"]]
        verdicts = [rec["result"]] + [t["result"] for t in rec["tampered"]]
        assert 1 in verdicts and 0 in verdicts, rec["n"]
        assert "32 bytes short" in names and "32 bytes long" in names
        if rec["n"]:
            assert {"message bit flipped", "r_i >= p", "r_i not an x coordinate", "key does not parse", "s >= n", "s off by one"} <= set(names)
        else:
            assert "n = 0, s = 1" in names and rec["agg"] == "00" * 32
        assert ("two items swapped" in names) == (rec["n"] >= 2)
    assert os.path.getsize(os.path.join(HERE, "golden", "halfagg_batch_vectors.json")) < 1 << 20


@pytest.mark.parametrize("pk_format", [0, 1])
def test_every_vector_alone(emu, pk_format):
    """a batch of ONE aggregate per vector"""
    for c in H.cases():
        H.check_verify(_verify(emu), [c], pk_format)


@pytest.mark.parametrize("pk_format", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_batches_at_a_wavefront_edge(emu, m, pk_format):
    H.check_verify(_verify(emu), H.of_count(m), pk_format)


@pytest.mark.parametrize("m", [63, 64, 65])
def test_exactly_m_chain_lanes(emu, m):
    """every aggregate of the batch owns a chain lane: the plan has exactly 63, 64 and 65 lanes (verification and aggregation)"""
    batch = H.with_lanes(m)
    keys, msgs, item_off, aggs, agg_off, _ = H.pack_verify(batch, 0)
    plan = np.zeros(3, np.uint64)
    emu.emu_halfagg_plan(_p(plan), _p(item_off), _p(agg_off), ctypes.c_size_t(m), ctypes.c_uint64(H.MM_MAX_TERMS))
    assert [int(x) for x in plan] == [m, m, 0]
    for f in (0, 1):
        H.check_verify(_verify(emu), batch, f)
    H.check_aggregate(_inc(emu), H.good_with_lanes(m), m & 1)


@pytest.mark.parametrize("pk_format", [0, 1])
def test_shuffled_batch(emu, pk_format):
    """every kind of refused aggregate next to accepted ones, item_off[k] odd and even"""
    batch = H.shuffled()
    assert sum(c.result for c in batch) == 8
    H.check_verify(_verify(emu), batch, pk_format)


def test_partition_at_a_small_limit(emu):
    """limit 8: aggregates of 5 and more signatures take the single-aggregate path next to 2-signature ones"""
    batch = H.shuffled()
    keys, msgs, item_off, aggs, agg_off, _ = H.pack_verify(batch, 0)
    plan = np.zeros(3, np.uint64)
    emu.emu_halfagg_plan(_p(plan), _p(item_off), _p(agg_off), ctypes.c_size_t(len(batch)), ctypes.c_uint64(8))
    right_len = [c for c in batch if len(c.agg) == 32 * (c.n + 1)]
    assert int(plan[2]) == sum(c.n >= 5 for c in right_len) > 0 and int(plan[0]) == sum(1 <= c.n <= 4 for c in right_len) == int(plan[1]) > 0
    for f in (0, 1):
        H.check_verify(_verify(emu, 8), batch, f)


def test_repeated_triple_at_the_real_limit(emu):
    big = H.repeated()
    by = {c.name: c for c in H.cases()}
    batch = [by["n=2"], big, by["n=2 s off by one"]]
    keys, msgs, item_off, aggs, agg_off, _ = H.pack_verify(batch, 0)
    plan = np.zeros(3, np.uint64)
    emu.emu_halfagg_plan(_p(plan), _p(item_off), _p(agg_off), ctypes.c_size_t(3), ctypes.c_uint64(H.MM_MAX_TERMS))
    assert [int(x) for x in plan] == [2, 2, 1]
    H.check_verify(_verify(emu), batch, 0)


@pytest.mark.parametrize("pk_format", [0, 1])
def test_aggregation_against_the_reference(emu, pk_format):
    good = H.good()
    H.check_aggregate(_inc(emu), good, pk_format)
    H.check_aggregate(_inc(emu), [good[i] for i in (7, 0, 3, 1, 6, 2, 5, 4)], pk_format)
    H.check_aggregate_refusals(_inc(emu), pk_format)


def test_aggregate_of_the_repeated_triple(emu):
    big = H.repeated()
    H.check_aggregate(_inc(emu), [big], 0)


def test_emulation_refuses_illegal_arguments(emu):
    b = np.zeros(4096, np.uint8); r = np.zeros(4, np.int32)
    good, start1, down = np.array([0, 1, 2], np.uint64), np.array([1, 1, 2], np.uint64), np.array([0, 2, 1], np.uint64)
    aoff = np.array([0, 64, 128], np.uint64)
    n2 = ctypes.c_size_t(2); lim = ctypes.c_uint64(8192)
    assert emu.emu_halfagg_verify_batch(_p(r), _p(b), 0, _p(b), _p(good), _p(b), _p(aoff), n2, lim) == 1
    for args in ((None, _p(b), 0, _p(b), _p(good), _p(b), _p(aoff)), (_p(r), None, 0, _p(b), _p(good), _p(b), _p(aoff)), (_p(r), _p(b), 0, None, _p(good), _p(b), _p(aoff)),
                 (_p(r), _p(b), 0, _p(b), None, _p(b), _p(aoff)), (_p(r), _p(b), 0, _p(b), _p(good), None, _p(aoff)), (_p(r), _p(b), 0, _p(b), _p(good), _p(b), None),
                 (_p(r), _p(b), 2, _p(b), _p(good), _p(b), _p(aoff)), (_p(r), _p(b), 0, _p(b), _p(start1), _p(b), _p(aoff)), (_p(r), _p(b), 0, _p(b), _p(down), _p(b), _p(aoff)),
                 (_p(r), _p(b), 0, _p(b), _p(good), _p(b), _p(down))):
        assert emu.emu_halfagg_verify_batch(*args, n2, lim) == 0, args
    nb_ok, nb_bad = np.array([1, 0], np.uint64), np.array([1, 2], np.uint64)
    assert emu.emu_halfagg_inc_aggregate_batch(_p(r), _p(b), _p(b), _p(nb_ok), _p(b), 0, _p(b), _p(b), _p(good), n2) == 1
    assert emu.emu_halfagg_inc_aggregate_batch(_p(r), _p(b), _p(b), _p(nb_bad), _p(b), 0, _p(b), _p(b), _p(good), n2) == 0
    assert emu.emu_halfagg_inc_aggregate_batch(_p(r), _p(b), _p(b), _p(nb_ok), _p(b), 0, _p(b), _p(b), _p(down), n2) == 0
    assert emu.emu_halfagg_aggregate_batch(_p(r), _p(b), _p(b), 0, _p(b), None, _p(good), n2) == 0


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib, api
    assert "engine_halfagg_batch" in build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "DIFFERENCE FROM THE REFERENCE: the aggregate's" in hdr and "Out of scope: group forms of these calls" in hdr
    for name in ("schnorrsig_aggverify_batch", "schnorrsig_aggregate_batch", "schnorrsig_inc_aggregate_batch"):
        assert callable(getattr(api.Engine, name))


def test_library_exports_and_argument_checks():
    """the built library: a missing one is a failed build, never a reason to skip.  The argument checks run before the engine is touched,
    so a placeholder engine pointer is enough to reach them without a device (every call below is one that must be refused)."""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    b = np.zeros(4096, np.uint8); bp = _p(b)
    e = _p(np.zeros(1 << 16, np.uint8))
    good, start1, down = _p(np.array([0, 1, 2], np.uint64)), _p(np.array([1, 1, 2], np.uint64)), _p(np.array([0, 2, 1], np.uint64))
    aoff = _p(np.array([0, 64, 128], np.uint64))
    nb_ok, nb_bad = _p(np.array([1, 0], np.uint64)), _p(np.array([1, 2], np.uint64))
    for pre, sfx in (((), ""), ((None,), "_dev")):
        v = getattr(lib, "secp256k1_schnorrsig_aggverify_batch" + sfx)
        a = getattr(lib, "secp256k1_schnorrsig_aggregate_batch" + sfx)
        i = getattr(lib, "secp256k1_schnorrsig_inc_aggregate_batch" + sfx)
        assert v(None, *pre, bp, bp, 0, bp, good, bp, aoff, 2) == 0 and "null engine" in _native.last_error()
        assert a(None, *pre, bp, bp, bp, 0, bp, bp, good, 2) == 0 and "null engine" in _native.last_error()
        assert i(None, *pre, bp, bp, bp, nb_ok, bp, 0, bp, bp, good, 2) == 0 and "null engine" in _native.last_error()
        for args in ((None, bp, 0, bp, good, bp, aoff), (bp, None, 0, bp, good, bp, aoff), (bp, bp, 0, None, good, bp, aoff), (bp, bp, 0, bp, None, bp, aoff),
                     (bp, bp, 0, bp, good, None, aoff), (bp, bp, 0, bp, good, bp, None), (bp, bp, -1, bp, good, bp, aoff), (bp, bp, 2, bp, good, bp, aoff),
                     (bp, bp, 0, bp, start1, bp, aoff), (bp, bp, 0, bp, down, bp, aoff), (bp, bp, 0, bp, good, bp, start1), (bp, bp, 0, bp, good, bp, down)):
            assert v(e, *pre, *args, 2) == 0 and lib.s2k_last_status() == 2, ("verify" + sfx, args)
        for args in ((None, bp, bp, 0, bp, bp, good), (bp, None, bp, 0, bp, bp, good), (bp, bp, None, 0, bp, bp, good), (bp, bp, bp, 0, None, bp, good),
                     (bp, bp, bp, 0, bp, None, good), (bp, bp, bp, 0, bp, bp, None), (bp, bp, bp, 2, bp, bp, good), (bp, bp, bp, 0, bp, bp, start1), (bp, bp, bp, 0, bp, bp, down)):
            assert a(e, *pre, *args, 2) == 0 and lib.s2k_last_status() == 2, ("aggregate" + sfx, args)
        for args in ((None, bp, bp, nb_ok, bp, 0, bp, bp, good), (bp, None, bp, nb_ok, bp, 0, bp, bp, good), (bp, bp, None, nb_ok, bp, 0, bp, bp, good),
                     (bp, bp, bp, None, bp, 0, bp, bp, good), (bp, bp, bp, nb_ok, None, 0, bp, bp, good), (bp, bp, bp, nb_ok, bp, 0, None, bp, good),
                     (bp, bp, bp, nb_ok, bp, 0, bp, None, good), (bp, bp, bp, nb_ok, bp, 0, bp, bp, None), (bp, bp, bp, nb_ok, bp, 3, bp, bp, good),
                     (bp, bp, bp, nb_ok, bp, 0, bp, bp, start1), (bp, bp, bp, nb_ok, bp, 0, bp, bp, down), (bp, bp, bp, nb_bad, bp, 0, bp, bp, good)):
            assert i(e, *pre, *args, 2) == 0 and lib.s2k_last_status() == 2, ("inc_aggregate" + sfx, args)


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    ok = dict(pubkeys=[bytes(64)], msgs32=[bytes(64)], aggsigs=[bytes(96)], pk_format=0)
    for bad in (dict(pk_format=2), dict(pubkeys=[bytes(63)]), dict(msgs32=[bytes(33)]), dict(pubkeys=None), dict(aggsigs=[]), dict(aggsigs=None), dict(msgs32=[bytes(64)] * 2),
                dict(pk_format=1)):
        with pytest.raises(ValueError):
            e.schnorrsig_aggverify_batch(**{**ok, **bad})
    ok = dict(pubkeys=[bytes(64)], msgs32=[bytes(64)], sigs64=[bytes(128)], pk_format=0)
    for bad in (dict(pk_format=-1), dict(sigs64=[bytes(64)]), dict(sigs64=[bytes(127)]), dict(sigs64=None), dict(pubkeys=[bytes(32)]), dict(sigs64=[bytes(128)] * 2)):
        with pytest.raises(ValueError):
            e.schnorrsig_aggregate_batch(**{**ok, **bad})
    ok = dict(aggsigs_in=[bytes(64)], pubkeys=[bytes(64)], msgs32=[bytes(64)], new_sigs64=[bytes(64)], pk_format=0)
    for bad in (dict(aggsigs_in=[bytes(63)]), dict(aggsigs_in=[bytes(0)]), dict(aggsigs_in=[bytes(128)]), dict(new_sigs64=[bytes(128)]), dict(aggsigs_in=[]), dict(pk_format=5)):
        with pytest.raises(ValueError):
            e.schnorrsig_inc_aggregate_batch(**{**ok, **bad})


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_schnorrsig_aggverify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_schnorrsig_aggverify_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_schnorrsig_aggregate_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_schnorrsig_aggregate_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_schnorrsig_inc_aggregate_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_schnorrsig_inc_aggregate_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "halfagg_batch.c"), "-o", str(tmp_path / "e.o")], check=True)


def test_docs_cover_the_batch_calls():
    for path in ("include/secp256k1_zkp_amd.h", "README.md", "DESIGN.md", "SURVEY.md"):
        assert "aggverify_batch" in open(os.path.join(ROOT, path)).read(), path
