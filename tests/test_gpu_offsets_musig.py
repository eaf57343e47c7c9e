"""GPU: where the MuSig2 family places an item in a batch (csrc/engine_core.hip: secp256k1_musig_partial_sig_verify_batch_group;
csrc/engine_lanes.h: lanes_run; csrc/engine_musig.hip).  Group shares that start at lo > 0 and launches that start at i0 > 0, at every
signature, nonce and key width and in both session modes.  The pools and the helpers are those of tests/test_gpu_musig.py; the verdicts
and sessions are the Python model's (tests/musig_ref.py).  tests/batch_edges.py asserts before every call that the batch could show a
wrong stride or a dropped offset."""
import ctypes

import numpy as np
import pytest

from tests import batch_edges as E
from tests import musig_ref as M
from tests.test_gpu_musig import KEY_BYTES, NONCE_BYTES, SIG_BYTES, _cut, _dev, _fmt, _names, _u8, pool, ppool  # noqa: F401  (pool, ppool: fixtures)

pytestmark = pytest.mark.gpu

GROUP_SIZES = (1, 2, 3, 4, 5, 65, 257, 599)
VERIFY_FORMATS = ((0, 0, 0), (1, 1, 1), (0, 1, 2), (1, 0, 0))


@pytest.fixture(scope="module")
def prows(pool):
    """the pool's shares as verify rows, which also carry the object forms of what parses (M.make_vrow: the model gives one verdict in
    every format combination the row exists in, and it is the pool's)"""
    caches, sessions, items = pool
    rows = []
    for i, (sig, nonce, pk, of, v) in enumerate(items):
        s = int.from_bytes(sig, "big"); R = (M.parse33(nonce[:33]), M.parse33(nonce[33:])); Pp = M.parse33(pk)
        r = M.make_vrow("share %d" % i, caches[of], sessions[of], sig_ser=sig, sig_o=M.sig_obj(s) if s < M.N else None, nonce_ser=nonce,
                        nonce_o=None if M.BAD in R else M.pubnonce_obj(*R), pk_ser=pk, pk_o=None if Pp == M.BAD else M.pt_obj(Pp))
        assert r[9] == v
        rows.append(r)
    return rows


@pytest.fixture(scope="module")
def ppool1(ppool):
    """the process pool with aggregate-nonce objects: (aggnonce132, msg32, cache197, adaptor64, (verdict, session) without the adaptor,
    (verdict, session) with it), the model's answers for the object; None where the serialised nonce does not parse"""
    out = []
    for an, msg, cache, ad, _, _ in ppool:
        R = (M.parse_ext(an[:33]), M.parse_ext(an[33:]))
        if M.BAD in R:
            out.append(None)
            continue
        o = M.aggnonce_obj(*R)
        out.append((o, msg, cache, ad, M.process_bytes(o, 1, msg, cache), M.process_bytes(o, 1, msg, cache, ad)))
    assert sum(x is not None for x in out) >= 80
    return out


@pytest.fixture(scope="module")
def groups():
    """three engines on device 0 (shares start at n/3 and 2n/3, and are empty below three items), and two engines on two devices where
    there are two"""
    import torch
    from secp256k1_zkp_amd import Group
    made = []
    try:
        made.append(Group([0, 0, 0]))
        made.append(Group([0, 1] if torch.cuda.device_count() > 1 else [0, 0]))
        yield made
    finally:
        for g in made:
            g.close()


def _cutf(prows, n, start, f):
    """_cut in the format combination f: the shares among n (cyclically from `start`) that exist in it -> (kept rows, sigs, nonces, pks,
    session_of, expected, after how many kept shares the batch repeats itself)"""
    idx = [(start + i) % len(prows) for i in range(n)]
    a = {j: M.verify_formats(prows[j], *f) for j in set(idx)}
    idx = [j for j in idx if a[j] is not None]
    return ([prows[j] for j in idx], _u8([a[j][0] for j in idx], SIG_BYTES[f[0]]), _u8([a[j][1] for j in idx], NONCE_BYTES[f[1]]), _u8([a[j][2] for j in idx], KEY_BYTES[f[2]]),
            np.array([j % 8 for j in idx], np.uint32), np.array([prows[j][9] for j in idx], np.int32), sum(1 for j in range(len(prows)) if M.verify_formats(prows[j], *f) is not None))


def test_group_shares(groups, pool, prows):
    """groups of three and of two engines: every share but the first starts at lo > 0, where the `_group` form adds sgb * lo (32, 36),
    nb * lo (66, 132) and pkb * lo (33, 64, 65) to the caller's arrays.  With session_of the eight pairs stay where they are and
    session_of + lo goes on; with one pair per share 197 * lo and 133 * lo are added as well.  599 shares put the starts at 199 and 399
    (at 299), which neither the pool's period nor the eight sessions divide; 1 .. 5 shares leave engines idle and give every engine
    other sessions.  The verdicts are the pool's."""
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    for f in VERIFY_FORMATS:
        for n in GROUP_SIZES if f == (0, 0, 0) else (599, 4):
            kept, sigs, nonces, pks, of, exp, period = _cutf(prows, n, 5, f)
            m = len(kept)
            assert m == n if f == (0, 0, 0) else m >= (560 if n == 599 else n - 1)
            assert all(caches[of[i]].tobytes() == kept[i][7] and sessions[of[i]].tobytes() == kept[i][8] for i in range(m))
            for g in groups:
                what = (f, n, len(g)); starts = E.share_starts(m, len(g))
                # (65 and 257 shares on two engines start the second share at 32 and 128: share t and share lo + t are on the same session)
                same_pairs = ("of", "caches", "sessions") if n < 599 and any(b % 8 == 0 for b in starts) else ()
                E.check(what, starts, dict(sigs=sigs, nonces=nonces, pks=pks, of=of, caches=caches[of], sessions=sessions[of]), exp, period=period, both=m >= 65, fixed=same_pairs)
                got = g.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=of, **_fmt(f))
                assert np.array_equal(got, exp), (what, "session_of", np.flatnonzero(got != exp)[:8], _names(kept, got, exp)[:4])
                got = g.musig_partial_sig_verify(sigs, nonces, pks, caches[of], sessions[of], **_fmt(f))
                assert np.array_equal(got, exp), (what, "one pair per share", np.flatnonzero(got != exp)[:8], _names(kept, got, exp)[:4])


def test_group_argument_checks(groups, pool):
    """a NULL array, a format out of range, and a session index >= n_sessions in the last share, through the `_group` form: 0 with the
    argument status, and nothing marked valid"""
    g = groups[0]; L = g._lib; h = g._h
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    it, sigs, nonces, pks, of, exp = _cut(pool, 6)
    assert exp.all()
    res = np.full(6, 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    good = [p(res), p(sigs), 0, p(nonces), 0, p(pks), 0, p(caches), p(sessions), 8, p(of), 6]
    assert L.secp256k1_musig_partial_sig_verify_batch_group(h, *good) == 1 and np.array_equal(res, exp)
    bad_of = of.copy(); bad_of[5] = 8                                                     # (three engines: the last share is items 4 and 5)
    for k, bad in ((0, None), (1, None), (3, None), (5, None), (7, None), (8, None), (2, 2), (2, -1), (4, 2), (4, -1), (6, 3), (6, -1), (9, 0), (10, None), (10, p(bad_of))):
        a = list(good); a[k] = bad; res[:] = 7                                            # (session_of NULL needs n_sessions == n)
        assert L.secp256k1_musig_partial_sig_verify_batch_group(h, *a) == 0 and L.s2k_last_status() == 2 and not (res == 1).any(), (k, bad)
    with pytest.raises(Exception):
        g.musig_partial_sig_verify(sigs, nonces, pks, caches, sessions, session_of=bad_of)
    assert L.secp256k1_musig_partial_sig_verify_batch_group(h, None, None, 0, None, 0, None, 0, None, None, 0, None, 0) == 1


def test_sub_range_launches_object_formats(pool, prows, ppool1):
    """700 items (less the few whose flipped bit left them without an object form) on an engine whose launches take 256 and then 512
    lanes, in the formats whose items are 36, 132, 64 and 65 bytes wide: verification with the pairs shared through session_of and with
    one pair per share (the pair arrays then move with the sub-range), nonce processing with 132-byte aggregate nonces, with and
    without adaptors.  Host and _dev form, against the pool's verdicts and the model's sessions."""
    import torch
    from secp256k1_zkp_amd import Engine
    caches, sessions = _u8(pool[0], 197), _u8(pool[1], 133)
    formats = ((1, 1, 1), (0, 1, 2))
    objs = [_cutf(prows, 700, 3, f) for f in formats]
    pkept = [x for x in (ppool1[i % len(ppool1)] for i in range(700)) if x is not None]
    pm1 = len(pkept); pperiod = sum(x is not None for x in ppool1)
    assert pm1 >= 600 and all(len(o[0]) >= 660 for o in objs)
    pn1, pmsg, pc1, pa1 = _u8([x[0] for x in pkept], 132), _u8([x[1] for x in pkept], 32), _u8([x[2] for x in pkept], 197), _u8([x[3] for x in pkept], 64)
    eng = Engine(0)
    try:
        for lanes in (256, 512):
            eng.set_option(Engine.OPT_MAX_LANES, lanes)
            for f, (kept, fs, fn, fp, fo, fexp, period) in zip(formats, objs):
                m = len(kept)
                E.check((f, lanes), E.launch_starts(m, lanes), dict(sigs=fs, nonces=fn, pks=fp, of=fo, caches=caches[fo], sessions=sessions[fo]), fexp, period=period)
                got = eng.musig_partial_sig_verify(fs, fn, fp, caches, sessions, session_of=fo, **_fmt(f))
                assert np.array_equal(got, fexp), (f, lanes, "session_of", _names(kept, got, fexp)[:4])
                got = eng.musig_partial_sig_verify(fs, fn, fp, caches[fo], sessions[fo], **_fmt(f))
                assert np.array_equal(got, fexp), (f, lanes, "one pair per share", _names(kept, got, fexp)[:4])
                d_a, d_b = (torch.full((m,), 7, dtype=torch.int32, device="cuda:0") for _ in range(2))
                t = [_dev(x) for x in (fs, fn, fp, caches, sessions, fo.view(np.int32), caches[fo], sessions[fo])]      # (held until the engine's stream has drained)
                eng.musig_partial_sig_verify_dev(d_a, t[0], t[1], t[2], t[3], t[4], 8, session_of=t[5], **_fmt(f))
                eng.musig_partial_sig_verify_dev(d_b, t[0], t[1], t[2], t[6], t[7], m, **_fmt(f))
                eng.sync()
                assert np.array_equal(d_a.cpu().numpy(), fexp) and np.array_equal(d_b.cpu().numpy(), fexp), (f, lanes, "dev")
            for k, ads in ((4, None), (5, pa1)):
                exp_v, exp_s = np.array([x[k][0] for x in pkept], np.int32), _u8([x[k][1] for x in pkept], 133)
                arrays = dict(nonces=pn1, msgs=pmsg, caches=pc1) if ads is None else dict(nonces=pn1, msgs=pmsg, caches=pc1, adaptors=pa1)
                # (what makes a serialised nonce fail leaves it without an object: every kept item reads 1, and its 133 session bytes are what is compared)
                E.check(("process", k, lanes), E.launch_starts(pm1, lanes), arrays, exp_v, period=pperiod, both=False)
                got = eng.musig_nonce_process(pn1, pmsg, pc1, adaptors=ads, nonce_format=1)
                assert np.array_equal(got[0], exp_v) and np.array_equal(got[1].reshape(pm1, 133), exp_s), (k, lanes)
                d_res = torch.full((pm1,), 7, dtype=torch.int32, device="cuda:0"); d_out = torch.full((pm1, 133), 0xEE, dtype=torch.uint8, device="cuda:0")
                t = [_dev(x) for x in (pn1, pmsg, pc1)] + [None if ads is None else _dev(ads)]
                eng.musig_nonce_process_dev(d_res, d_out, t[0], t[1], t[2], adaptors=t[3], nonce_format=1)
                eng.sync()
                assert np.array_equal(d_res.cpu().numpy(), exp_v) and np.array_equal(d_out.cpu().numpy(), exp_s), (k, lanes, "dev")
    finally:
        eng.set_option(Engine.OPT_MAX_LANES, 1 << 20)
        eng.close()
