"""CPU tier: MuSig2 partial-signature verification and nonce processing.  secp256k1_zkp_amd/csrc/musig.h runs on the host
(tests/host_emul/musig_emu.cpp, S2K_VERIFY on, 12-bit generator table) against the Python model of tests/musig_ref.py and the recorded
rows (tests/golden/musig_vectors.json: the verdicts and sessions of the reference's own secp256k1_musig_partial_sig_verify and
secp256k1_musig_nonce_process, the module's BIP-327 vectors among them); plus the midstates, the ABI, the argument checks and the C example."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import musig_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MUSIG_SYMBOLS = ["secp256k1_musig_partial_sig_verify_batch", "secp256k1_musig_partial_sig_verify_batch_dev", "secp256k1_musig_partial_sig_verify_batch_group",
                 "secp256k1_musig_partial_sig_verify_amd", "secp256k1_musig_nonce_process_batch", "secp256k1_musig_nonce_process_batch_dev"]


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(HERE, "host_emul", "libs2k_musig_emu.so")
    assert os.path.exists(path), "tests/host_emul/libs2k_musig_emu.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(path)
    cp, ci = ctypes.c_char_p, ctypes.c_int
    lib.emu_musig_verify.argtypes = [cp, ci, cp, ci, cp, ci, cp, cp]
    lib.emu_musig_verify_indexed.argtypes = [cp, ci, cp, ci, cp, ci, cp, cp, ctypes.c_size_t, ctypes.c_uint]
    lib.emu_musig_joint_count.restype = ctypes.c_ulonglong
    lib.emu_musig_process.argtypes = [cp, cp, ci, cp, cp, cp]
    lib.emu_musig_midstates.argtypes = [cp]
    return lib


@pytest.fixture(scope="module")
def golden():
    j = json.load(open(os.path.join(HERE, "golden", "musig_vectors.json")))
    return M.from_json(j["verify"], M.VERIFY_INPUTS), M.from_json(j["process"], M.PROCESS_INPUTS)


@pytest.fixture(scope="module")
def edge():
    return M.edge_cases()


def _emu_verify(emu, r, f):
    a = M.verify_formats(r, *f)
    return None if a is None else emu.emu_musig_verify(a[0], f[0], a[1], f[1], a[2], f[2], r[7], r[8])


def _emu_process(emu, r, nf):
    n = M.process_formats(r, nf)
    if n is None:
        return None
    out = ctypes.create_string_buffer(b"\xee" * 133, 133)
    return emu.emu_musig_process(out, n, nf, r[3], r[4], r[5]), out.raw


def test_golden_fixture_shape(golden):
    V, Pr = golden
    for rows in (V, Pr):
        names = [r[0] for r in rows]
        assert len(set(names)) == len(names) and sum(1 for x in names if x.startswith("random ")) == 64
    assert 100 <= len(V) <= 160 and 80 <= len(Pr) <= 160
    v = {r[0]: r[9] for r in V}
    assert [v["BIP-327 sign/verify valid %d" % i] for i in range(4)] == [1] * 4 and [v["BIP-327 tweak valid %d" % i] for i in range(5)] == [1] * 5
    assert sum(1 for nm in v if nm.startswith("BIP-327 verify fail")) == 3 and sum(1 for nm in v if nm.startswith("BIP-327 verify error")) == 2
    assert all(x == 0 for nm, x in v.items() if nm.startswith(("BIP-327 verify fail", "BIP-327 verify error")))
    assert all(len(r[7]) == 197 and len(r[8]) == 133 for r in V) and all(len(r[4]) == 197 and len(r[7]) == 133 for r in Pr)
    assert all(r[7] == bytes(133) for r in Pr if r[6] == 0) and all(r[7][:4] == M.MAGIC_SESSION for r in Pr if r[6] == 1)
    rnd = [r for r in V if r[0].startswith("random ")]
    assert all(r[9] == 1 for i, r in enumerate(rnd) if i % 4 != 3) and any(r[9] == 0 for r in rnd)


def test_model_against_fixture(golden):
    """the Python model returns the reference's recorded verdict and session on every row, in every format the row exists in"""
    V, Pr = golden
    for r in V:
        for f in M.ALL_VERIFY_FORMATS:
            a = M.verify_formats(r, *f)
            if a is not None:
                assert M.verify_bytes(a[0], f[0], a[1], f[1], a[2], f[2], r[7], r[8]) == r[9], (r[0], f)
    for r in Pr:
        for nf in (0, 1):
            n = M.process_formats(r, nf)
            if n is not None:
                assert M.process_bytes(n, nf, r[3], r[4], r[5]) == (r[6], r[7]), (r[0], nf)


def test_edge_lists_are_the_recorded_ones(golden, edge):
    """the edge lists rebuilt now are the recorded ones, each item has the verdict its name promises, and the list holds what it must"""
    V, Pr = golden
    assert edge[0] == [r for r in V if not r[0].startswith(("random ", "BIP-327 "))]
    assert edge[1] == [r for r in Pr if not r[0].startswith(("random ", "BIP-327 "))]
    names = {r[0] for r in edge[0]}
    assert set(M.EDGE_VERDICTS) <= names and len(names) == len(edge[0])
    for r in edge[0]:
        assert r[9] == M.EDGE_VERDICTS.get(r[0], 0), r[0]
    for need in ("s + 1", "s = 0", "serialised s = n", "object s = n", "wrong magic: partial signature", "wrong magic: pubnonce", "wrong magic: cache",
                 "wrong magic: session", "all-zero key object", "compressed key: x >= p", "compressed key: x off the curve", "compressed key: prefix 04",
                 "serialised pubnonce: R1 invalid", "serialised pubnonce: R2 invalid", "serialised pubnonce: 33 zero bytes", "T infinite alone",
                 "J == T (the doubling in the last comparison)", "R1 = s*G"):
        assert need in names, need
    pn = {r[0]: r for r in edge[1]}
    assert set(M.EDGE_PROCESS_FAILS) <= set(pn) and len(pn) == len(edge[1])
    for r in edge[1]:
        assert r[6] == (0 if r[0] in M.EDGE_PROCESS_FAILS else 1), r[0]
    g = M.G[0].to_bytes(32, "big")
    for name in ("both aggregate points infinite (the final nonce is G)", "adaptor = -R1, R2 infinite (the final nonce is G)"):
        assert pn[name][7][5:37] == g and pn[name][7][4] == (M.G[1] & 1), name
    # the shapes of the cache: zero and non-zero tweak, each with an aggregate key of odd and of even y
    seen = {(M.cache_unpack(r[4])["tweak"] != 0, M.cache_unpack(r[4])["pk"][1] & 1) for r in edge[1] if r[0].startswith("cache ")}
    assert len(seen) == 4
    # object-only and serialised-only rows are exactly the ones the formats cannot express
    assert {r[0] for r in edge[0] if r[1] is None or r[3] is None or r[5] is None} == {
        "object s = n", "object s = n, valid as 0", "wrong magic: partial signature", "wrong magic: pubnonce", "all-zero key object"}
    assert {r[0] for r in edge[0] if r[2] is None or r[4] is None or r[6] is None} == {
        "serialised s = n", "serialised s = n where 0 is valid", "compressed key: x >= p", "compressed key: x off the curve", "compressed key: prefix 04",
        "serialised pubnonce: R1 invalid", "serialised pubnonce: R2 invalid", "serialised pubnonce: 33 zero bytes"}


def test_emu_golden_every_format_and_coverage(emu, golden):
    """the recorded rows through the host-emulated lane routines in every format combination a row exists in.  Coverage: every row runs
    in at least one combination, and every combination runs at least 80 % of the rows"""
    V, Pr = golden
    j0 = emu.emu_musig_joint_count()
    per_row = [0] * len(V)
    for f in M.ALL_VERIFY_FORMATS:
        ran = 0
        for i, r in enumerate(V):
            got = _emu_verify(emu, r, f)
            if got is not None:
                assert got == r[9], (r[0], f)
                ran += 1; per_row[i] += 1
        assert ran >= 0.8 * len(V), (f, ran)
    assert min(per_row) >= 1
    assert emu.emu_musig_joint_count() - j0 >= 12 * 80                                    # the joint form is what ordinary items take
    per_row = [0] * len(Pr)
    for nf in (0, 1):
        ran = 0
        for i, r in enumerate(Pr):
            got = _emu_process(emu, r, nf)
            if got is not None:
                assert got[0] == r[6], (r[0], nf)
                assert got[1] == r[7], (r[0], nf, "session bytes")
                ran += 1; per_row[i] += 1
        assert ran >= 0.8 * len(Pr), (nf, ran)
    assert min(per_row) >= 1


def test_emu_joint_counter(emu, edge):
    """ordinary items take the joint form; the fallback rows (a zero scalar, R2 = -P meeting its own x, dead items) take the two-call
    form with the same verdicts"""
    rows = {r[0]: r for r in edge[0]}
    for name in ("signer is the second key (mu = 1)", "signer is the first key", "cache both tweaks, aggregate key odd", "R2 = P", "s = 0, valid"):
        j0 = emu.emu_musig_joint_count()
        assert _emu_verify(emu, rows[name], (0, 0, 0)) == 1
        assert emu.emu_musig_joint_count() == j0 + 1, name
    for name in M.FALLBACK_ROWS + ("R2 = -P", "J infinite alone", "b' = -e', R2 = P, s*G = sigma*R1: J and T infinite, valid"):
        j0 = emu.emu_musig_joint_count()
        assert _emu_verify(emu, rows[name], (0, 0, 0)) == rows[name][9]
        assert emu.emu_musig_joint_count() == j0, name


def test_emu_random_against_model(emu):
    """96 seeded rows of each kind, one in four with a flipped bit, and shares on shared sessions through session_of"""
    V, Pr = M.random_items(96, 6603)
    assert 64 <= sum(r[9] for r in V) < 96
    for r in V:
        assert _emu_verify(emu, r, (0, 0, 0)) == r[9], r[0]
    for r in V[:24]:
        for f in ((1, 1, 1), (0, 1, 2), (1, 0, 1)):
            got = _emu_verify(emu, r, f)
            assert got is None or got == r[9], (r[0], f)
    for r in Pr:
        assert _emu_process(emu, r, 0) == (r[6], r[7]), r[0]
    caches, sessions, items = M.shared_pool(24, 6604, n_sessions=4, signers=3, corrupt_every=4)
    cs, ss = b"".join(caches), b"".join(sessions)
    assert 0 < sum(x[4] for x in items) < 24
    for sig, nonce, pk, S, verdict in items:
        assert emu.emu_musig_verify_indexed(sig, 0, nonce, 0, pk, 0, cs, ss, 4, S) == verdict
    sig, nonce, pk, S, verdict = items[0]
    assert verdict == 1 and emu.emu_musig_verify_indexed(sig, 0, nonce, 0, pk, 0, cs, ss, 4, 4) == 0      # an index past the pairs: 0, nothing read
    assert emu.emu_musig_verify_indexed(sig, 0, nonce, 0, pk, 0, cs, ss, 4, (S + 1) % 4) == 0


def test_midstates_against_hashlib(emu):
    """the three midstates the engine computes with its own SHA-256 are the states after the tag hashes twice: pinned through digests
    (a wrong midstate cannot give hashlib's digest of tag | tag | message) and, for the two the reference keeps as constants
    (keyagg_impl.h:93-99, session_impl.h:535-541), word for word"""
    mid = ctypes.create_string_buffer(96); emu.emu_musig_midstates(mid)
    words = lambda b: [int.from_bytes(b[4 * i:4 * i + 4], "big") for i in range(8)]      # noqa: E731
    assert words(mid.raw[0:32]) == [0x6ef02c5a, 0x06a480de, 0x1f298665, 0x1d1134f2, 0x56a0b063, 0x52da4147, 0xf280d9d4, 0x4484be15]
    assert words(mid.raw[32:64]) == [0x2c7d5a45, 0x06bf7e53, 0x89be68a6, 0x971254c0, 0x60ac12d2, 0x72846dcd, 0x6c81212f, 0xde7a2500]
    assert len(set((mid.raw[0:32], mid.raw[32:64], mid.raw[64:96]))) == 3
    # through the lane routine: a session's b and e are the tagged hashes of the model's byte strings
    rng = np.random.default_rng(6605)
    sc = M.Scenario(rng, [M._rand_scalar(rng) for _ in range(2)])
    out = ctypes.create_string_buffer(133)
    assert emu.emu_musig_process(out, M.aggnonce_ser(*sc.agg), 0, sc.msg, sc.cache, None) == 1
    pkx = M.b32(M.cache_unpack(sc.cache)["pk"][0])
    t = hashlib.sha256(b"MuSig/noncecoef").digest()
    assert int.from_bytes(out.raw[37:69], "big") == int.from_bytes(hashlib.sha256(t + t + M.aggnonce_ser(*sc.agg) + pkx + sc.msg).digest(), "big") % M.N
    t = hashlib.sha256(b"BIP0340/challenge").digest()
    assert int.from_bytes(out.raw[69:101], "big") == int.from_bytes(hashlib.sha256(t + t + out.raw[5:37] + pkx + sc.msg).digest(), "big") % M.N


def test_abi_is_declared():
    from secp256k1_zkp_amd import _native, build_lib
    assert "engine_musig" in build_lib.UNITS_ADDED
    hdr = open(os.path.join(ROOT, "include", "secp256k1_zkp_amd.h")).read()
    for name in MUSIG_SYMBOLS:
        assert name in _native.SIGNATURES and ("S2K_API int %s(" % name) in hdr, name
    assert "133 zero bytes" in hdr and "illegal-argument callback" in hdr                 # the two deliberate differences are documented


def test_library_exports_musig():
    """the built library: a missing one is a failed build (hipcc cross-compiles it without a GPU), never a reason to skip"""
    from secp256k1_zkp_amd import _native
    assert os.path.exists(_native.LIB_PATH), _native.LIB_PATH + " not built (python -c 'import __graft_entry__ as g; g.build()')"
    lib = _native.load()
    for name in MUSIG_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.secp256k1_musig_partial_sig_verify_batch(None, None, None, 0, None, 0, None, 0, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_musig_partial_sig_verify_batch_dev(None, None, None, None, 0, None, 0, None, 0, None, None, 1, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_musig_partial_sig_verify_batch_group(None, None, None, 0, None, 0, None, 0, None, None, 1, None, 1) == 0 and "null group" in _native.last_error()
    assert lib.secp256k1_musig_nonce_process_batch(None, None, None, None, 0, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    assert lib.secp256k1_musig_nonce_process_batch_dev(None, None, None, None, None, 0, None, None, None, 1) == 0 and "null engine" in _native.last_error()
    # the single-item form: NULL where the reference has ARG_CHECK is an illegal argument before any device is touched
    o = ctypes.create_string_buffer(b"\x01" * 197, 197)
    for k in range(5):
        args = [o] * 5; args[k] = None
        assert lib.secp256k1_musig_partial_sig_verify_amd(None, *args) == 0 and lib.s2k_last_status() == 2


def test_python_argument_checks():
    """the size and format checks run before anything reaches the library (no engine needed: the methods are called on a bare object)"""
    from secp256k1_zkp_amd import api
    e = api.Engine.__new__(api.Engine)
    g = api.Group.__new__(api.Group)
    ok = dict(partial_sigs=bytes(32), pubnonces=bytes(66), pubkeys=bytes(33), keyagg_caches=bytes(197), sessions=bytes(133))
    for obj in (e, g):
        for bad in (dict(sig_format=2), dict(nonce_format=-1), dict(pk_format=3), dict(sig_format=1), dict(nonce_format=1), dict(pk_format=1),
                    dict(partial_sigs=bytes(31)), dict(pubnonces=bytes(65)), dict(keyagg_caches=bytes(196)), dict(sessions=bytes(132)), dict(pubkeys=None),
                    dict(sessions=bytes(266), keyagg_caches=bytes(394)),                 # two pairs for one share without session_of
                    dict(session_of=np.zeros(2, np.uint32))):
            with pytest.raises(ValueError):
                obj.musig_partial_sig_verify(**{**ok, **bad})
    for bad in (dict(nonce_format=2), dict(aggnonces=bytes(65)), dict(msgs32=bytes(31)), dict(keyagg_caches=bytes(198)), dict(adaptors=bytes(63)), dict(aggnonces=None)):
        with pytest.raises(ValueError):
            e.musig_nonce_process(**{**dict(aggnonces=bytes(66), msgs32=bytes(32), keyagg_caches=bytes(197)), **bad})


def test_header_and_example_are_plain_c(tmp_path):
    inc = "-I" + os.path.join(ROOT, "include")
    src = tmp_path / "t.c"
    src.write_text('#include "secp256k1_zkp_amd.h"\nint main(void) { return secp256k1_musig_partial_sig_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'secp256k1_musig_partial_sig_verify_amd(0, 0, 0, 0, 0, 0) + secp256k1_musig_nonce_process_batch(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", inc, "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", inc, "-c", os.path.join(ROOT, "examples", "musig_verify.c"), "-o", str(tmp_path / "e.o")], check=True)
