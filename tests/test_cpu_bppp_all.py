"""CPU tier of the one-verdict BP++ norm-argument verifier: csrc/bppp_all.h compiled for the host (tests/host_emul/bppp_all_emu.cpp) and
driven in the order engine_bppp_all.hip launches its kernels -- the level plan, the column-sum plan, the node array, the passes of the
column sums -- against the derivation written with hashlib and the sums recomputed with Python integers (tests/bppp_all_ref.py), the
reference's prover and verifier, its 13 verification vectors, cancelling changes and batches whose points coincide; the C ABI's argument
checks, the Python size checks and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import bppp_all_cases as C
from tests import bppp_all_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ["secp256k1_bppp_norm_product_verify_all", "secp256k1_bppp_norm_product_verify_all_dev"]
_sz = ctypes.c_size_t


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_bppp_all_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_bppp_all_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_bppp_all_chunk.restype = ctypes.c_uint
    return lib


@pytest.fixture(scope="module")
def tw(ref):
    from tests import tweak_ref
    return tweak_ref.TweakRef()


def _batch_args(batch):
    """the thirteen input arguments the emulation's entry points share (arrays kept alive by the caller's tuple)"""
    proofs, trs, rhos, gens, g_len, cvs, commits = batch
    n = rhos.size // 32
    arrs = [np.ascontiguousarray(x, np.uint8) for x in (proofs, trs, rhos, gens, cvs, commits)]
    pr, tr, rh, ge, cv, cm = arrs
    nz = lambda a: _p(a) if n else None
    return arrs, (nz(pr), _sz(pr.size // max(n, 1)), nz(tr), nz(rh), _p(ge), _sz(ge.size // 33), _sz(g_len), nz(cv), _sz(cv.size // 32 // max(n, 1)), nz(cm), _sz(n))


def _call(emu, max_terms=0):
    def call(batch, locate):
        keep, args = _batch_args(batch)
        n = batch[2].size // 32
        v = np.full(1, -7, np.int32); res = np.full(max(n, 1), -7, np.int32) if locate else None; seed = np.full(32, 0xEE, np.uint8)
        assert emu.emu_bppp_verify_all(_p(v), _p(res), _p(seed), *args, _sz(max_terms)) == 1
        return int(v[0]), (res[:n] if locate else None), seed.tobytes()
    return call


def _seed(emu, batch):
    keep, args = _batch_args(batch)
    n = batch[2].size // 32
    seed = np.full(32, 0xEE, np.uint8); co = np.full((max(n, 1), 16), 0xEE, np.uint8); zp = np.full((max(n, 1), 32), 0xEE, np.uint8)
    assert emu.emu_bppp_all_seed(_p(seed), _p(co), _p(zp), *args) == 1
    ints = lambda a: [int.from_bytes(a[i].tobytes(), "big") for i in range(n)]
    return seed.tobytes(), ints(co), ints(zp)


def test_level_plan_and_column_sum_plan(emu):
    L = emu.emu_bppp_all_chunk()
    assert L >= 2
    for n in sorted({0, 1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097, L - 1, L, L + 1, 16 * L, 16 * L + 1, 256 * L + 1}):
        counts = np.zeros(24, np.uint64); cc = np.zeros(24, np.uint64); out4 = np.zeros(4, np.uint64); totals = np.zeros(2, np.uint64)
        levels = emu.emu_bppp_all_plan(_p(counts), _p(cc), _p(out4), _p(totals), _sz(n), 24)
        want, cwant = R.level_plan(n), R.colsum_plan(n, L)
        assert [int(x) for x in counts[:levels]] == want and int(totals[0]) == sum(want), n
        assert int(out4[0]) == len(want) and int(out4[2]) == L, n
        assert [int(x) for x in cc[:int(out4[1])]] == cwant and int(out4[3]) == sum(cwant[:-1]), n
    assert R.colsum_plan(L, L) == [1, 1] and R.colsum_plan(L + 1, L) == [2, 1] and R.colsum_plan(16 * L + 1, L) == [17, 2, 1]


@pytest.mark.parametrize("shape", [(4, 4), (64, 8)])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 255, 256, 257])
def test_seed_and_coefficients_against_hashlib(emu, n, shape):
    batch = C.random_batch(shape, n)
    seed, co, zp = _seed(emu, batch)
    want = R.seed(*batch)
    assert seed == want
    assert co == R.coefficients(want, n) and co[0] == 1 and all(0 < z < 1 << 128 for z in co)
    assert zp == R.zprime(want, n)


def test_seed_depends_on_every_input(emu):
    batch = C.random_batch((4, 4), 257)
    seen = {_seed(emu, batch)[0]}
    for which, idx in ((0, (0, 3)), (0, (256, 193)), (1, (15, 100)), (1, (16, 0)), (2, (255, 31)), (5, (17, 3, 7)), (6, (256, 32)), (3, (0, 0)), (3, (7, 32))):
        b = C.copy(batch); b[which][idx] ^= 1
        seed = _seed(emu, b)[0]
        assert seed == R.seed(*b) and seed not in seen, (which, idx)
        seen.add(seed)
    short = tuple(x[:256] if k not in (3, 4) else x for k, x in enumerate(batch))
    assert _seed(emu, short)[0] not in seen                                                 # and on n
    assert R.gens_digest(batch[3], 4) != R.gens_digest(batch[3], 2)


@pytest.mark.parametrize("shape", [(1, 1), (2, 8), (64, 8)])
def test_scalars_against_python_integers(emu, shape):
    """sc[p][t] as bp_prologue and bp_sg_entry leave them; z'_p, S_t, g_sc and the own-term scalars recomputed from those"""
    L = emu.emu_bppp_all_chunk()
    g_len, h_len = shape
    n_gens, own = g_len + h_len, 2 * C.n_rounds(*shape) + 1
    n_terms = n_gens + 1 + own
    for n in (1, 17, L + 1):
        batch = C.random_batch(shape, n, seed=5)
        batch[0][:, -64] &= 0x7F; batch[0][:, -32] &= 0x7F                                  # n, l below the group order
        keep, args = _batch_args(batch)
        sc = np.full((n, n_terms, 32), 0xEE, np.uint8); zp = np.full((n, 32), 0xEE, np.uint8); S = np.full((n_gens, 32), 0xEE, np.uint8)
        g = np.full(32, 0xEE, np.uint8); ow = np.full((n, own, 32), 0xEE, np.uint8); inf = np.full(n_gens + n * own, 0xEE, np.uint8)
        assert emu.emu_bppp_all_scalars(_p(sc), _p(zp), _p(S), _p(g), _p(ow), _p(inf), *args) in (0, 1)
        i = lambda b: int.from_bytes(b.tobytes(), "big")
        sc_i = [[i(sc[p, t]) for t in range(n_terms)] for p in range(n)]
        zp_i = [i(zp[p]) for p in range(n)]
        assert zp_i == R.zprime(R.seed(*batch), n)
        assert all(row[n_gens + 1] == R.N - 1 for row in sc_i) and all(0 < v < R.N for row in sc_i for v in row)
        wS, wg, wown = R.sums(sc_i, zp_i, n_gens)
        assert [i(S[t]) for t in range(n_gens)] == wS and i(g) == wg
        assert [[i(ow[p, j]) for j in range(own)] for p in range(n)] == wown
        assert set(inf.tolist()) <= {0, 1}


@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_valid_batches(emu, ref, shape, n):
    C.check_valid(_call(emu), ref, shape, n)


@pytest.mark.parametrize("shape,n", [((4, 4), 5), ((2, 8), 3)])
def test_one_corruption(emu, ref, shape, n):
    C.check_corrupted(_call(emu), ref, shape, n)


def test_reference_vectors(emu, ref):
    C.check_vectors(_call(emu), ref)


@pytest.mark.parametrize("n", [2, 17])
def test_cancelling_changes_are_caught(emu, ref, tw, n):
    C.check_cancellation(_call(emu), ref, tw, (4, 4), n)


def test_coincident_points(emu, ref):
    C.check_coincident(_call(emu), ref)


def test_infinity_encodings(emu, ref):
    C.check_infinity_encodings(_call(emu), ref)


def test_empty_batch_rejected_shape_and_batch_too_large(emu, ref):
    C.check_empty(_call(emu))
    good = C.valid_batch(ref, (4, 4), 5)
    bad_shape = (good[0], good[1], good[2], good[3], 2, good[5], good[6])                   # g_len + h_len != n_gens
    v, res, seed = _call(emu)(bad_shape, True)
    assert v == 0 and res.tolist() == [0] * 5 and seed == bytes(32)
    assert _call(emu)((good[0][:, :-1], *good[1:]), False)[0] == 0                           # proof_len
    # 8 generators + 5 points a proof: 33 points and G
    assert _call(emu, 34)(good, False)[0] == 1
    keep, args = _batch_args(good)
    v = np.zeros(1, np.int32)
    assert emu.emu_bppp_verify_all(_p(v), None, None, *args, _sz(33)) == 0


def test_emulation_refuses_illegal_arguments(emu):
    batch = C.random_batch((4, 4), 1)
    keep, args = _batch_args(batch)
    v = np.zeros(1, np.int32)
    assert emu.emu_bppp_verify_all(_p(v), None, None, *args, _sz(0)) == 1
    assert emu.emu_bppp_verify_all(None, None, None, *args, _sz(0)) == 0
    for k in (0, 2, 3, 4, 7, 9):
        a = list(args); a[k] = None
        assert emu.emu_bppp_verify_all(_p(v), None, None, *a, _sz(0)) == 0, k


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib, api
    assert "engine_bppp_all" in build_lib.UNITS_ADDED and build_lib.UNITS_ADDED.index("engine_bppp_all") < build_lib.UNITS_ADDED.index("engine_musig_agg")
    assert os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "engine_bppp_all.hip")) and os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "bppp_all.h"))
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in SYMBOLS + ["s2k_bppp_all_last_split_ms"]:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "S2K/bppp_all/item" in hdr and "beyond the fill level" in hdr and "2^-128" in hdr
    assert callable(api.Engine.bppp_norm_product_verify_all) and callable(api.Engine.bppp_norm_product_verify_all_dev) and callable(api.Engine.bppp_all_last_split_ms)


def test_library_exports_and_argument_checks():
    """the built library: a missing one is a failed build, never a reason to skip.  The argument checks run before the engine is touched,
    so a placeholder engine pointer is enough to reach them without a device (every call below is one that must be refused)."""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in SYMBOLS + ["s2k_bppp_all_last_split_ms"]:
        assert hasattr(lib, name), name
    b = np.zeros(4096, np.uint8); bp = _p(b)
    e = _p(np.zeros(1 << 16, np.uint8))
    host, dev = lib.secp256k1_bppp_norm_product_verify_all, lib.secp256k1_bppp_norm_product_verify_all_dev
    ok = [bp, 194, bp, bp, bp, 8, 4, bp, 4, bp]                          # proofs, proof_len, transcripts, rho, gens33, n_gens, g_len, c_vec, c_vec_len, commits33
    assert host(None, bp, None, None, *ok, 1) == 0 and "null engine" in _native.last_error()
    assert dev(None, None, bp, None, *ok[:5], bp, *ok[5:], 1) == 0 and "null engine" in _native.last_error()
    assert lib.s2k_bppp_all_last_split_ms(None, bp) == 0 and "null engine" in _native.last_error()
    for k in (None, 0, 2, 3, 4, 7, 9):
        a = list(ok); verdict = bp
        if k is None:
            verdict = None
        else:
            a[k] = None
        lib.s2k_clear_status()
        assert host(e, verdict, None, None, *a, 1) == 0 and lib.s2k_last_status() == 2, ("host", k)
        lib.s2k_clear_status()
        assert dev(e, None, verdict, None, *a[:5], bp, *a[5:], 1) == 0 and lib.s2k_last_status() == 2, ("dev", k)
    lib.s2k_clear_status()
    assert dev(e, None, bp, None, *ok[:5], None, *ok[5:], 1) == 0 and lib.s2k_last_status() == 2             # gens33_host


def test_python_size_checks():
    """the size checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    ok = dict(proofs=bytes(2 * 194), transcripts=bytes(208), rho=bytes(64), gens33=bytes(8 * 33), g_len=4, c_vec=bytes(2 * 4 * 32), commits33=bytes(66))
    for bad in (dict(proofs=None), dict(transcripts=None), dict(rho=None), dict(gens33=None), dict(c_vec=None), dict(commits33=None), dict(proofs=bytes(2 * 194 + 1)),
                dict(transcripts=bytes(207)), dict(rho=bytes(63)), dict(gens33=bytes(8 * 33 - 1)), dict(c_vec=bytes(2 * 4 * 32 + 32)), dict(commits33=bytes(65)),
                dict(g_len=-1), dict(proofs=bytes(0)), dict(c_vec=bytes(0)), dict(gens33=bytes(0))):
        with pytest.raises(ValueError):
            e.bppp_norm_product_verify_all(**{**ok, **bad})

    class T:                                          # what the _dev form asks of a tensor
        def __init__(self, n): self.n = n
        def numel(self): return self.n
        def data_ptr(self): return 0
    ok = dict(verdict=T(1), proofs=T(2 * 194), proof_len=194, transcripts=T(208), rho=T(64), gens33_dev=T(8 * 33), gens33_host=bytes(8 * 33), g_len=4, c_vec=T(256),
              c_vec_len=4, commits33=T(66), n=2)
    for bad in (dict(verdict=None), dict(verdict=T(0)), dict(seed_out=T(31)), dict(proofs=T(387)), dict(transcripts=T(207)), dict(rho=T(63)), dict(c_vec=T(255)),
                dict(commits33=T(65)), dict(gens33_dev=T(8 * 33 - 1)), dict(gens33_host=None), dict(gens33_host=bytes(8 * 33 + 1)), dict(n=3), dict(n=-1), dict(proofs=None)):
        with pytest.raises(ValueError):
            e.bppp_norm_product_verify_all_dev(**{**ok, **bad})


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_bppp_norm_product_verify_all(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_bppp_norm_product_verify_all_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + s2k_bppp_all_last_split_ms(0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "bppp_verify_all.c"), "-o", str(tmp_path / "e.o")], check=True)


def test_docs_cover_the_call():
    for path in ("include/secp256k1_zkp_amd.h", "README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "bppp_norm_product_verify_all" in open(os.path.join(ROOT, path)).read(), path
    assert "eighteen translation units" in open(os.path.join(ROOT, "README.md")).read()
