"""CPU tier of the MuSig2 aggregation calls: csrc/musig_agg.h compiled for the host (tests/host_emul/musig_agg_emu.cpp), driven the
way engine_musig_agg.hip plans its stages, against the recorded answers of the reference (tests/golden/musig_agg_vectors.json) and
the model (tests/musig_agg_ref.py) on every edge and random row, in every format combination and at fan-in 2, 3 and 64; the
"KeyAgg list" midstate against the reference's constant; the C ABI, the Python argument checks and the C example."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import musig_agg_ref as A
from tests import musig_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH = ["secp256k1_musig_pubkey_agg_batch", "secp256k1_musig_pubkey_tweak_add_batch", "secp256k1_musig_nonce_agg_batch", "secp256k1_musig_partial_sig_agg_batch"]
SYMBOLS = BATCH + [s + "_dev" for s in BATCH] + ["secp256k1_musig_pubkey_agg_amd"]
FANINS = (2, 3, 64)
N_IN = (A.KEYAGG_INPUTS, A.TWEAK_INPUTS, A.NONCE_INPUTS, A.SIG_INPUTS)
NAMES = ("keyagg", "tweak", "nonce_agg", "sig_agg")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def _off(counts):
    off = np.zeros(len(counts) + 1, np.uint64)
    off[1:] = np.cumsum(counts)
    return off


class Emu:
    """the batch forms of the emulation; outputs start as 0xEE"""

    def __init__(self, lib):
        self.lib = lib

    def keyagg(self, sets, pk_format, fanin=64, want_agg=True):
        n = len(sets); off = _off([len(s) // A.PK_BYTES[pk_format] for s in sets])
        r = np.full(n, -1, np.int32); c = np.full(197 * n, 0xEE, np.uint8); a = np.full(64 * n, 0xEE, np.uint8)
        assert self.lib.emu_musig_pubkey_agg(_p(r), _p(c), _p(a) if want_agg else None, _p(_u8(b"".join(sets))), pk_format, _p(off), ctypes.c_size_t(n), fanin) == 1
        return [(int(r[k]), c[197 * k:197 * k + 197].tobytes(), a[64 * k:64 * k + 64].tobytes()) for k in range(n)]

    def tweak(self, caches, tweaks, xonly, in_place=False):
        n = len(caches); r = np.full(n, -1, np.int32); cin = _u8(b"".join(caches)); out = cin if in_place else np.full(197 * n, 0xEE, np.uint8)
        pk = np.full(64 * n, 0xEE, np.uint8)
        assert self.lib.emu_musig_pubkey_tweak_add(_p(r), _p(out), _p(pk), _p(cin), _p(_u8(b"".join(tweaks))), None if xonly is None else _p(np.array(xonly, np.uint8)),
                                                   ctypes.c_size_t(n)) == 1
        return [(int(r[k]), out[197 * k:197 * k + 197].tobytes(), pk[64 * k:64 * k + 64].tobytes()) for k in range(n)]

    def nonce_agg(self, sessions, nonce_format, out_format, fanin=64):
        n = len(sessions); nb, ob = (132 if nonce_format else 66), (132 if out_format else 66)
        off = _off([len(s) // nb for s in sessions]); r = np.full(n, -1, np.int32); o = np.full(ob * n, 0xEE, np.uint8)
        assert self.lib.emu_musig_nonce_agg(_p(r), _p(o), out_format, _p(_u8(b"".join(sessions))), nonce_format, _p(off), ctypes.c_size_t(n), fanin) == 1
        return [(int(r[k]), o[ob * k:ob * k + ob].tobytes()) for k in range(n)]

    def sig_agg(self, sessions, sigs, sig_format):
        n = len(sessions); sb = 36 if sig_format else 32
        off = _off([len(s) // sb for s in sigs]); r = np.full(n, -1, np.int32); o = np.full(64 * n, 0xEE, np.uint8)
        assert self.lib.emu_musig_partial_sig_agg(_p(r), _p(o), _p(_u8(b"".join(sessions))), _p(_u8(b"".join(sigs))), sig_format, _p(off), ctypes.c_size_t(n)) == 1
        return [(int(r[k]), o[64 * k:64 * k + 64].tobytes()) for k in range(n)]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_musig_agg_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_musig_agg_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    lib.emu_musig_agg_plan.restype = ctypes.c_size_t
    return Emu(lib)


@pytest.fixture(scope="module")
def golden_json():
    return json.load(open(os.path.join(HERE, "golden", "musig_agg_vectors.json")))


@pytest.fixture(scope="module")
def golden(golden_json):
    return tuple(A.from_json(golden_json[NAMES[w]], w, N_IN[w]) for w in range(4))


def test_golden_fixture_shape(golden):
    K, T, Nn, S = golden
    for w, rows in enumerate(golden):
        names = [r[0] for r in rows]
        assert len(set(names)) == len(names)
        assert sum(n.startswith("random ") for n in names) == 64 and any(n.startswith("BIP-327") for n in names)
    for edges, rows in ((A.keyagg_edges(), K), (A.tweak_edges(), T), (A.nonce_edges(), Nn), (A.sig_edges(), S)):
        assert {r[0] for r in edges} <= {r[0] for r in rows}
    assert sum(r[0].startswith("BIP-327 key_agg valid") for r in K) == 4 and sum(r[0].startswith("BIP-327 key_agg error") for r in K) == 5
    assert os.path.getsize(os.path.join(HERE, "golden", "musig_agg_vectors.json")) < 1 << 20


def test_model_against_fixture(golden):
    """every recorded answer is what the model says, in every byte and in every representation the row exists in"""
    K, T, Nn, S = golden
    for r in K:
        for f in range(3):
            if r[1 + f] is not None:
                assert A.keyagg_bytes(r[1 + f], f) == tuple(r[4:]), (r[0], f)
    for r in T:
        assert A.tweak_bytes(r[1], r[2], r[3]) == tuple(r[4:]), r[0]
    for r in Nn:
        for f in range(2):
            if r[1 + f] is not None:
                assert A.nonce_agg_bytes(r[1 + f], f) == tuple(r[3:]), (r[0], f)
    for r in S:
        for f in range(2):
            if r[2 + f] is not None:
                assert A.sig_agg_bytes(r[1], r[2 + f], f) == tuple(r[4:]), (r[0], f)


def test_edge_verdicts_are_the_documented_ones(golden):
    """served and refused as the header documents, by the reference's recorded verdicts"""
    K, T, Nn, S = ({r[0]: r for r in rows} for rows in golden)
    for r in A.keyagg_edges():
        assert K[r[0]][4] == (0 if r[0] in A.KEYAGG_EDGE_REFUSED else 1), r[0]
    for r in A.tweak_edges():
        assert T[r[0]][4] == (0 if A._tweak_refused(r[0]) else 1), r[0]
    for r in A.nonce_edges():
        assert Nn[r[0]][3] == (0 if r[0] in A.NONCE_EDGE_REFUSED else 1), r[0]
    for r in A.sig_edges():
        assert S[r[0]][4] == (0 if r[0] in A.SIG_EDGE_REFUSED else 1), r[0]
    # the shapes: second_pk infinite, second key at index 2, infinite aggregate nonces, the grouped model against the plain one
    assert K["all keys equal (second infinite, all doublings)"][5][68:132] == bytes(64)
    P0, Q = A._edge_points()[1][:2]
    assert K["[P, P, Q]: the second key is index 2"][5][68:132] == M.pt_obj(Q)
    assert K["key 1 a hybrid encoding of key 0's point, Q after it"][5] == K["[P, P, Q]: the second key is index 2"][5]
    assert K["[P, Q, P, Q, R]"][5] == M.pubkey_agg([P0, Q, P0, Q, A._edge_points()[1][2]])
    assert Nn["R and -R in the first column only"][4][:33] == bytes(33) and Nn["R and -R in the first column only"][4][33:] != bytes(33)
    assert Nn["R and -R in both columns"][4] == bytes(66) and Nn["R and -R in both columns"][5] == M.MAGIC_AGGNONCE + bytes(128)
    assert S["object s = n (reduced)"][4] == 1 and S["object s = n (reduced)"][5][32:] == M.b32(5)


@pytest.mark.parametrize("fanin", FANINS)
def test_emu_keyagg_golden_every_format(emu, golden, fanin):
    """all rows of a format as ONE batch (sets of every size side by side, refused sets between served ones), per fan-in"""
    for f in range(3):
        rows = [r for r in golden[0] if r[1 + f] is not None]
        assert len(rows) >= 60
        got = emu.keyagg([r[1 + f] for r in rows], f, fanin)
        for r, g in zip(rows, got):
            assert g == tuple(r[4:]), (r[0], f, fanin)


def test_emu_keyagg_plan_and_single_sets(emu):
    """the plan: passes = ceil(log_fanin(max m)), at least one; and each edge set alone (a batch of one) without the x-only output"""
    for m, fanin, passes in ((1, 64, 1), (64, 64, 1), (65, 64, 2), (130, 64, 2), (2, 2, 1), (3, 2, 2), (8, 2, 3), (9, 2, 4), (9, 3, 2), (0, 2, 1)):
        off = np.array([0, m, m, m + 1], np.uint64); cap = ctypes.c_size_t(0)
        assert emu.lib.emu_musig_agg_plan(_p(off), ctypes.c_size_t(3), fanin, ctypes.byref(cap)) == passes, (m, fanin)
        assert cap.value == max(m + 1, 3)
    for r in A.keyagg_edges()[:20]:
        for f in range(3):
            if r[1 + f] is not None:
                n = len(r[1 + f]) // A.PK_BYTES[f]; off = _off([n]); res = np.full(1, -1, np.int32); c = np.full(197, 0xEE, np.uint8)
                assert emu.lib.emu_musig_pubkey_agg(_p(res), _p(c), None, _p(_u8(r[1 + f])), f, _p(off), ctypes.c_size_t(1), 2) == 1
                assert (int(res[0]), c.tobytes()) == tuple(r[4:6]), (r[0], f)


def test_emu_keyagg_pool_against_model(emu):
    """the pool of the batch tests: the recipe's conditions on the inputs, then the emulation against the model"""
    pool = A.keyagg_pool()
    assert all(p[3][0] == 1 for p in pool)                                                      # every uncorrupted set is served
    assert sum(1 for p in pool if p[1] and p[2][0] == 0) >= 4                                   # corrupted: refused ...
    assert sum(1 for p in pool if p[1] and p[2][0] == 1 and p[2][1] != p[3][1]) >= 4            # ... or served with another cache
    for fanin in (2, 64):
        got = emu.keyagg([p[0] for p in pool], 0, fanin)
        assert got == [p[2] for p in pool]


def test_emu_tweak(emu, golden):
    rows = golden[1]
    for in_place in (False, True):
        got = emu.tweak([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], in_place)
        for r, g in zip(rows, got):
            assert g == tuple(r[4:]), (r[0], in_place)
    plain = [r for r in rows if r[3] == 0]                                                      # xonly NULL: all plain
    assert emu.tweak([r[1] for r in plain], [r[2] for r in plain], None) == [tuple(r[4:]) for r in plain]


@pytest.mark.parametrize("fanin", FANINS)
def test_emu_nonce_agg_every_format(emu, golden, fanin):
    for nf in range(2):
        rows = [r for r in golden[2] if r[1 + nf] is not None]
        for of in range(2):
            got = emu.nonce_agg([r[1 + nf] for r in rows], nf, of, fanin)
            for r, g in zip(rows, got):
                assert g == (r[3], r[4 + of]), (r[0], nf, of, fanin)


def test_emu_sig_agg_every_format(emu, golden):
    for sf in range(2):
        rows = [r for r in golden[3] if r[2 + sf] is not None]
        got = emu.sig_agg([r[1] for r in rows], [r[2 + sf] for r in rows], sf)
        for r, g in zip(rows, got):
            assert g == tuple(r[4:]), (r[0], sf)


def test_emu_random_against_model(emu):
    """rows the fixture does not hold"""
    K, T, Nn, S = A.random_rows(24, 6626)
    assert emu.keyagg([r[1] for r in K], 0, 3) == [tuple(r[4:]) for r in K]
    assert emu.tweak([r[1] for r in T], [r[2] for r in T], [r[3] for r in T]) == [tuple(r[4:]) for r in T]
    assert emu.nonce_agg([r[1] for r in Nn], 0, 1, 2) == [(r[3], r[5]) for r in Nn]
    assert emu.sig_agg([r[1] for r in S], [r[2] for r in S], 0) == [tuple(r[4:]) for r in S]


def test_list_midstate_against_the_reference_constant(emu, golden_json):
    out = ctypes.create_string_buffer(32)
    emu.lib.emu_musig_agg_list_midstate(out)
    words = [out.raw[4 * i:4 * i + 4].hex() for i in range(8)]
    assert words == golden_json["keyagg_list_midstate"] and len(words) == 8
    # ... and it is what the tag gives: a one-key list hashed from the midstate is the tagged hash
    P0 = A._edge_points()[1][0]
    t = hashlib.sha256(b"KeyAgg list").digest()
    assert A.keyagg_bytes(M.ser33(P0), 0)[1][132:164] == hashlib.sha256(t + t + M.ser33(P0)).digest()


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib, api
    assert "engine_musig_agg" in build_lib.UNITS_ADDED and build_lib.UNITS_ADDED[-1] == "engine_musig_agg"
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "#define S2K_OPT_MUSIG_SUM_FANIN 12" in hdr and api.Engine.OPT_MUSIG_SUM_FANIN == 12
    assert "197 zero bytes" in hdr and "VERIFY_CHECK" in hdr and "BIP-328" in hdr           # the differences and what is out of scope are documented
    for name in ("musig_pubkey_agg", "musig_pubkey_tweak_add", "musig_nonce_agg", "musig_partial_sig_agg"):
        assert callable(getattr(api.Engine, name)) and callable(getattr(api.Engine, name + "_dev"))
    # every exported declaration of the header has its ctypes entry
    import re
    for name in re.findall(r"S2K_API\s+[\w \*]+?\b(\w+)\(", hdr):
        assert name in _native.SIGNATURES, name


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
    calls = {
        "secp256k1_musig_pubkey_agg_batch": lambda en, st, res, out, f, off: lib.secp256k1_musig_pubkey_agg_batch(en, res, out, bp, bp, f, off, 2),
        "secp256k1_musig_pubkey_agg_batch_dev": lambda en, st, res, out, f, off: lib.secp256k1_musig_pubkey_agg_batch_dev(en, None, res, out, bp, bp, f, off, 2),
        "secp256k1_musig_nonce_agg_batch": lambda en, st, res, out, f, off: lib.secp256k1_musig_nonce_agg_batch(en, res, out, 0, bp, f, off, 2),
        "secp256k1_musig_nonce_agg_batch_dev": lambda en, st, res, out, f, off: lib.secp256k1_musig_nonce_agg_batch_dev(en, None, res, out, 0, bp, f, off, 2),
        "secp256k1_musig_partial_sig_agg_batch": lambda en, st, res, out, f, off: lib.secp256k1_musig_partial_sig_agg_batch(en, res, out, bp, bp, f, off, 2),
        "secp256k1_musig_partial_sig_agg_batch_dev": lambda en, st, res, out, f, off: lib.secp256k1_musig_partial_sig_agg_batch_dev(en, None, res, out, bp, bp, f, off, 2),
    }
    for name, call in calls.items():
        assert call(None, None, bp, bp, 0, good) == 0 and "null engine" in _native.last_error(), name
        for args in ((None, bp, 0, good), (bp, None, 0, good), (bp, bp, 0, None), (bp, bp, -1, good), (bp, bp, 3, good), (bp, bp, 0, start1), (bp, bp, 0, down)):
            assert call(e, None, *args) == 0 and lib.s2k_last_status() == 2, (name, args)
    assert lib.secp256k1_musig_nonce_agg_batch(e, bp, bp, 2, bp, 0, good, 2) == 0 and lib.s2k_last_status() == 2          # out_format
    assert lib.secp256k1_musig_nonce_agg_batch_dev(e, None, bp, bp, -1, bp, 0, good, 2) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_musig_pubkey_agg_batch(e, bp, bp, None, None, 0, good, 2) == 0 and lib.s2k_last_status() == 2     # keys missing
    for fn, pre in ((lib.secp256k1_musig_pubkey_tweak_add_batch, ()), (lib.secp256k1_musig_pubkey_tweak_add_batch_dev, (None,))):
        assert fn(None, *pre, bp, bp, bp, bp, bp, bp, 1) == 0 and "null engine" in _native.last_error()
        for k in (0, 1, 3, 4):                                                                 # results, caches_out, caches_in, tweaks32
            args = [bp] * 6; args[k] = None
            assert fn(e, *pre, *args, 1) == 0 and lib.s2k_last_status() == 2, k
    # the single-item form: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched
    o = ctypes.create_string_buffer(64); ptrs = (ctypes.c_void_p * 2)(ctypes.addressof(o), None)
    assert lib.secp256k1_musig_pubkey_agg_amd(None, o, o, None, 1) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_musig_pubkey_agg_amd(None, o, o, ptrs, 0) == 0 and lib.s2k_last_status() == 2
    assert lib.secp256k1_musig_pubkey_agg_amd(None, o, o, ptrs, 2) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    for bad in (dict(pk_format=3), dict(pubkeys=bytes(65)), dict(pubkeys=None), dict(set_off=[1, 2]), dict(set_off=[0, 2, 1]), dict(set_off=None), dict(set_off=[0, 3])):
        with pytest.raises(ValueError):
            e.musig_pubkey_agg(**{**dict(pubkeys=bytes(66), set_off=[0, 2], pk_format=0), **bad})
    for bad in (dict(keyagg_caches=bytes(196)), dict(tweaks32=bytes(33)), dict(xonly=bytes(2)), dict(tweaks32=None)):
        with pytest.raises(ValueError):
            e.musig_pubkey_tweak_add(**{**dict(keyagg_caches=bytes(197), tweaks32=bytes(32), xonly=bytes(1)), **bad})
    for bad in (dict(nonce_format=2), dict(out_format=-1), dict(pubnonces=bytes(131)), dict(nonce_off=[0, 1, 0]), dict(pubnonces=None)):
        with pytest.raises(ValueError):
            e.musig_nonce_agg(**{**dict(pubnonces=bytes(132), nonce_off=[0, 2]), **bad})
    for bad in (dict(sig_format=2), dict(sessions=bytes(132)), dict(partial_sigs=bytes(63)), dict(sig_off=[0, 1]), dict(sessions=None)):
        with pytest.raises(ValueError):
            e.musig_partial_sig_agg(**{**dict(sessions=bytes(133), partial_sigs=bytes(64), sig_off=[0, 2]), **bad})


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_musig_pubkey_agg_batch(0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_musig_pubkey_tweak_add_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_musig_nonce_agg_batch(0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_musig_partial_sig_agg_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0) + secp256k1_musig_pubkey_agg_amd(0, 0, 0, 0, 0) + S2K_OPT_MUSIG_SUM_FANIN; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "musig_keyagg.c"), "-o", str(tmp_path / "e.o")], check=True)


def test_docs_no_longer_leave_aggregation_to_the_reference():
    for path in ("include/secp256k1_zkp_amd.h", "secp256k1_zkp_amd/csrc/musig.h", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, path)).read()
        assert "musig_agg" in text or "pubkey_agg_batch" in text, path
        for stale in ("stay with the reference, as do key aggregation", "pubkey_agg and the cache tweaks (once per key set)"):
            assert stale not in text, (path, stale)
