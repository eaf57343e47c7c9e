"""CPU tier of the one-verdict BIP-340 batch verifier: csrc/schnorr_all.h compiled for the host (tests/host_emul/schnorr_all_emu.cpp) and
driven in the order engine_schnorr_all.hip launches its kernels -- the level plan, the node array, the passes of the scalar sum --
against the derivation written with hashlib (tests/schnorr_all_ref.py), the BIP-340 vectors, the reference's signer and verifier, and
batches whose points coincide; the C ABI's argument checks, the Python size checks and the C example."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import schnorr_all_cases as C
from tests import schnorr_all_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ["secp256k1_schnorrsig_verify_all", "secp256k1_schnorrsig_verify_all_dev"]
SIZES = [1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097]      # every tree-level boundary up to three levels


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_schnorr_all_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_schnorr_all_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    return ctypes.CDLL(path)


def _seed(emu, s, m, k, msglen, pk_format, want_coeffs=True):
    s, m, k = (np.ascontiguousarray(x, np.uint8) for x in (s, m, k))
    n = s.size // 64
    seed = np.full(32, 0xEE, np.uint8); co = np.full((max(n, 1), 16), 0xEE, np.uint8) if want_coeffs else None
    assert emu.emu_schnorr_all_seed(_p(seed), _p(co), _p(s), _p(m) if m.size else None, ctypes.c_size_t(msglen), _p(k), pk_format, ctypes.c_size_t(n)) == 1
    return seed.tobytes(), (None if co is None else [int.from_bytes(co[i].tobytes(), "big") for i in range(n)])


def _call(emu):
    def call(s, m, k, msglen, pk_format, locate):
        s, m, k = (np.ascontiguousarray(x, np.uint8) for x in (s, m, k))
        n = s.size // 64
        v = np.full(1, -7, np.int32); res = np.full(max(n, 1), -7, np.int32) if locate else None; seed = np.full(32, 0xEE, np.uint8)
        assert emu.emu_schnorr_verify_all(_p(v), _p(res), _p(seed), _p(s) if n else None, _p(m) if m.size else None, ctypes.c_size_t(msglen), _p(k) if n else None,
                                          pk_format, ctypes.c_size_t(n)) == 1
        return int(v[0]), (res[:n] if locate else None), seed.tobytes()
    return call


def test_level_plan(emu):
    for n, want in ((0, []), (1, [1]), (2, [2, 1]), (16, [16, 1]), (17, [17, 2, 1]), (256, [256, 16, 1]), (257, [257, 17, 2, 1]), (4096, [4096, 256, 16, 1]),
                    (4097, [4097, 257, 17, 2, 1]), (1 << 20, [1 << 20, 1 << 16, 4096, 256, 16, 1])):
        counts = np.zeros(24, np.uint64); totals = np.zeros(2, np.uint64)
        levels = emu.emu_schnorr_all_plan(_p(counts), _p(totals), ctypes.c_size_t(n), 24)
        assert [int(x) for x in counts[:levels]] == want == R.level_plan(n), n
        assert int(totals[0]) == sum(want) and int(totals[1]) == (n if n <= 1 else sum(want[1:])), n
    # 2^20 items: five launches of the node kernel
    assert len(R.level_plan(1 << 20)) - 1 == 5


@pytest.mark.parametrize("msglen", [0, 32, 33])
@pytest.mark.parametrize("n", SIZES)
def test_seed_and_coefficients_against_hashlib(emu, n, msglen):
    s, m, k = C.random_batch(n, msglen)
    seed, co = _seed(emu, s, m, k, msglen, 0)
    want = R.seed(s, m, k, msglen, 0)
    assert seed == want
    assert co == R.coefficients(want, n) and co[0] == 1 and all(0 < a < 1 << 128 for a in co)


def test_key_formats_give_the_same_seed(emu):
    """the digest hashes the key's 32 serialised bytes: for an object that is its x, whatever its y says"""
    for n in (1, 17, 257):
        s, m, k = C.random_batch(n, 32)
        obj = np.zeros((n, 64), np.uint8); obj[:, :32] = k[:, ::-1]; obj[:, 32:] = C.random_batch(n, 32, 9)[2]
        a, b = _seed(emu, s, m, k, 32, 0, False)[0], _seed(emu, s, m, obj, 32, 1, False)[0]
        assert a == b == R.seed(s, m, k, 32, 0) == R.seed(s, m, obj, 32, 1)


def test_seed_depends_on_every_item(emu):
    s, m, k = C.random_batch(257, 32)
    seen = {_seed(emu, s, m, k, 32, 0, False)[0]}
    for i in (0, 15, 16, 255, 256):
        m2 = m.copy(); m2[i, 31] ^= 1
        seed = _seed(emu, s, m2, k, 32, 0, False)[0]
        assert seed == R.seed(s, m2, k, 32, 0) and seed not in seen, i
        seen.add(seed)
    assert _seed(emu, s[:256], m[:256], k[:256], 32, 0, False)[0] not in seen                 # and on n


def _python_reference_is_bip340():
    """the restatement the others are pinned against: the vectors, and the batch equation on them"""
    for msglen, (good, bad) in C.vectors().items():
        for t in good:
            assert R.verify(*t) == 1
        for t in bad:
            assert R.verify(*t) == 0
        assert R.verify_all(*R.pack(good), msglen) == 1
        assert R.verify_all(*R.pack(good + bad[:1]), msglen) == 0 if bad else True


def test_bip340_vectors(emu):
    _python_reference_is_bip340()
    C.check_vectors(_call(emu))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_valid_batches(emu, ref, n):
    C.check_valid(_call(emu), ref, n)


@pytest.mark.parametrize("n", [2, 65])
def test_one_corruption(emu, ref, n):
    C.check_corrupted(_call(emu), ref, n)


@pytest.mark.parametrize("n", [2, 17, 65])
def test_cancelling_changes_are_caught(emu, ref, n):
    C.check_cancellation(_call(emu), ref, n)


def test_coincident_points(emu):
    C.check_coincident(_call(emu))


def test_empty_batch(emu):
    C.check_empty(_call(emu))
    seed = np.full(32, 0xEE, np.uint8)
    assert emu.emu_schnorr_all_seed(_p(seed), None, None, None, ctypes.c_size_t(32), None, 0, ctypes.c_size_t(0)) == 1 and seed.tobytes() == bytes(32)


def test_emulation_refuses_illegal_arguments(emu):
    b = np.zeros(4096, np.uint8); v = np.zeros(1, np.int32); n1 = ctypes.c_size_t(1); ml = ctypes.c_size_t(32)
    assert emu.emu_schnorr_verify_all(_p(v), None, None, _p(b), _p(b), ml, _p(b), 0, n1) == 1
    assert emu.emu_schnorr_verify_all(_p(v), None, None, _p(b), None, ctypes.c_size_t(0), _p(b), 0, n1) == 1
    for args in ((None, None, None, _p(b), _p(b), ml, _p(b), 0), (_p(v), None, None, None, _p(b), ml, _p(b), 0), (_p(v), None, None, _p(b), None, ml, _p(b), 0),
                 (_p(v), None, None, _p(b), _p(b), ml, None, 0), (_p(v), None, None, _p(b), _p(b), ml, _p(b), 2), (_p(v), None, None, _p(b), _p(b), ml, _p(b), -1)):
        assert emu.emu_schnorr_verify_all(*args, n1) == 0, args


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib, api
    assert build_lib.UNITS_ADDED[-2:] == ["engine_schnorr_all", "engine_musig_agg"]
    assert os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "engine_schnorr_all.hip")) and os.path.exists(os.path.join(ROOT, "secp256k1_zkp_amd", "csrc", "schnorr_all.h"))
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in SYMBOLS + ["s2k_schnorr_all_last_split_ms"]:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "S2K/schnorr_all/item" in hdr and "main_impl.h:215-261" in hdr and "2^-128" in hdr
    assert callable(api.Engine.schnorrsig_verify_all) and callable(api.Engine.schnorrsig_verify_all_dev)


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
    host, dev = lib.secp256k1_schnorrsig_verify_all, lib.secp256k1_schnorrsig_verify_all_dev
    assert host(None, bp, None, None, bp, bp, 32, bp, 0, 1) == 0 and "null engine" in _native.last_error()
    assert dev(None, None, bp, None, bp, bp, 32, bp, 0, 1) == 0 and "null engine" in _native.last_error()
    for args in ((None, bp, bp, 32, bp, 0), (bp, None, bp, 32, bp, 0), (bp, bp, None, 32, bp, 0), (bp, bp, bp, 32, None, 0), (bp, bp, bp, 32, bp, 2), (bp, bp, bp, 32, bp, -1)):
        verdict, rest = args[0], args[1:]
        lib.s2k_clear_status()
        assert host(e, verdict, None, None, *rest, 1) == 0 and lib.s2k_last_status() == 2, ("host", args)
        lib.s2k_clear_status()
        assert dev(e, None, verdict, None, *rest, 1) == 0 and lib.s2k_last_status() == 2, ("dev", args)


def test_python_size_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    ok = dict(sigs=bytes(128), msgs=bytes(64), pubkeys=bytes(64), msglen=32, pk_format=0)
    for bad in (dict(pk_format=2), dict(pk_format=-1), dict(sigs=bytes(127)), dict(msgs=bytes(63)), dict(msgs=bytes(64), msglen=33), dict(pubkeys=bytes(63)), dict(pk_format=1),
                dict(pubkeys=None), dict(sigs=None), dict(msgs=None), dict(msglen=0), dict(msglen=-1)):
        with pytest.raises(ValueError):
            e.schnorrsig_verify_all(**{**ok, **bad})

    class T:                                          # what the _dev form asks of a tensor
        def __init__(self, n): self.n = n
        def numel(self): return self.n
        def data_ptr(self): return 0
    ok = dict(verdict=T(1), sigs=T(128), msgs=T(64), pubkeys=T(64), msglen=32, pk_format=0)
    for bad in (dict(pk_format=3), dict(verdict=None), dict(verdict=T(0)), dict(seed_out=T(31)), dict(msgs=T(63)), dict(pubkeys=T(63)), dict(pk_format=1), dict(n=3)):
        with pytest.raises(ValueError):
            e.schnorrsig_verify_all_dev(**{**ok, **bad})


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_schnorrsig_verify_all(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_schnorrsig_verify_all_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + s2k_schnorr_all_last_split_ms(0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "schnorr_verify_all.c"), "-o", str(tmp_path / "e.o")], check=True)


def test_docs_cover_the_call():
    for path in ("include/secp256k1_zkp_amd.h", "README.md", "DESIGN.md", "SURVEY.md", "INTEGRATION.md"):
        assert "schnorrsig_verify_all" in open(os.path.join(ROOT, path)).read(), path
    assert "seventeen translation units" in open(os.path.join(ROOT, "README.md")).read()
