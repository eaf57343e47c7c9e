"""Host-side mirror of the reference's verify interfaces for the hot path, batch-shaped.

Names and argument meaning follow the reference (``secp256k1_ecmult``, ``secp256k1_ecmult_multi_var``,
``secp256k1_schnorrsig_verify``, ``secp256k1_rangeproof_verify``, ``secp256k1_bppp_rangeproof_norm_product_verify``);
each method returns per-item results equal to the reference's single-item call.  Inputs are numpy ``uint8`` arrays
(host path: staged through the engine's HBM workspace) or torch CUDA tensors (``*_dev`` path: already resident).
"""
import ctypes

import numpy as np

from . import _native


class S2KError(RuntimeError):
    pass


def _u8(a, shape=None):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _need(what, arr, nbytes):
    """host arrays reach hipMemcpy with sizes derived from n: a wrong-shaped argument must be an exception, not an out-of-bounds read"""
    if arr is None:
        raise ValueError(f"{what}: missing array")
    if arr.size != nbytes:
        raise ValueError(f"{what}: expected {nbytes} bytes, got {arr.size}")


def _offsets_ok(what, off, nbytes):
    off = np.asarray(off)
    if off.size == 0 or int(off[0]) != 0 or (np.diff(off.astype(np.int64)) < 0).any() or int(off[-1]) > nbytes:
        raise ValueError(f"{what}: offsets must start at 0, be non-decreasing and end inside the data ({nbytes} bytes)")


def _dp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_ECDSA_PK_BYTES = {0: 33, 1: 64, 2: 65}     # compressed / secp256k1_pubkey object / uncompressed or hybrid


def _ecdsa_args(what, sigs, msghashes, pubkeys, sig_format, pk_format):
    """shape checks shared by Engine.ecdsa_verify_batch and Group.ecdsa_verify_batch; returns (sigs, sig_off or None, msghashes, pubkeys, n)"""
    if sig_format not in (0, 1, 2) or pk_format not in _ECDSA_PK_BYTES:
        raise ValueError(f"{what}: sig_format must be 0, 1 or 2 and pk_format 0, 1 or 2")
    off = None
    if sig_format == 2:
        if isinstance(sigs, tuple) and len(sigs) == 2:
            data, off = _u8(sigs[0]), np.ascontiguousarray(sigs[1], dtype=np.uint64)       # already packed: (data, offsets[n+1])
        else:
            data, off = Engine.pack([bytes(x) for x in sigs])
        n = off.size - 1
        _offsets_ok(what + " sigs", off, data.size)
        sigs = data
    else:
        sigs = _u8(sigs); n = sigs.size // 64
        _need(what + " sigs", sigs, 64 * n)
    msghashes = _u8(msghashes); pubkeys = _u8(pubkeys)
    _need(what + " msghashes", msghashes, 32 * n); _need(what + " pubkeys", pubkeys, _ECDSA_PK_BYTES[pk_format] * n)
    return sigs, off, msghashes, pubkeys, n


def _adaptor_args(what, adaptor_sigs, pubkeys, msgs32, enckeys, pk_format):
    """shape checks shared by Engine.ecdsa_adaptor_verify_batch and Group.ecdsa_adaptor_verify_batch"""
    if pk_format not in _ECDSA_PK_BYTES:
        raise ValueError(f"{what}: pk_format must be 0, 1 or 2")
    if adaptor_sigs is None or pubkeys is None or msgs32 is None or enckeys is None:
        raise ValueError(f"{what}: missing array")
    adaptor_sigs = _u8(adaptor_sigs); pubkeys = _u8(pubkeys); msgs32 = _u8(msgs32); enckeys = _u8(enckeys); n = adaptor_sigs.size // 162
    _need(what + " adaptor_sigs", adaptor_sigs, 162 * n); _need(what + " msgs32", msgs32, 32 * n)
    _need(what + " pubkeys", pubkeys, _ECDSA_PK_BYTES[pk_format] * n); _need(what + " enckeys", enckeys, _ECDSA_PK_BYTES[pk_format] * n)
    return adaptor_sigs, pubkeys, msgs32, enckeys, n


def _musig_verify_args(what, partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, sig_format, nonce_format, pk_format):
    """shape checks shared by Engine.musig_partial_sig_verify and Group.musig_partial_sig_verify; returns the arrays, n_sessions and n"""
    if sig_format not in (0, 1) or nonce_format not in (0, 1) or pk_format not in _ECDSA_PK_BYTES:
        raise ValueError(f"{what}: sig_format and nonce_format must be 0 or 1 and pk_format 0, 1 or 2")
    if partial_sigs is None or pubnonces is None or pubkeys is None or keyagg_caches is None or sessions is None:
        raise ValueError(f"{what}: missing array")
    partial_sigs = _u8(partial_sigs); pubnonces = _u8(pubnonces); pubkeys = _u8(pubkeys); keyagg_caches = _u8(keyagg_caches); sessions = _u8(sessions)
    sgb = 36 if sig_format else 32
    n = partial_sigs.size // sgb; ns = sessions.size // 133
    _need(what + " partial_sigs", partial_sigs, sgb * n); _need(what + " pubnonces", pubnonces, (132 if nonce_format else 66) * n)
    _need(what + " pubkeys", pubkeys, _ECDSA_PK_BYTES[pk_format] * n)
    _need(what + " sessions", sessions, 133 * ns); _need(what + " keyagg_caches", keyagg_caches, 197 * ns)
    if session_of is None:
        if ns != n:
            raise ValueError(f"{what}: without session_of there is one cache and one session per item ({n}), got {ns}")
    else:
        session_of = np.ascontiguousarray(session_of, dtype=np.uint32)
        if session_of.size != n:
            raise ValueError(f"{what}: session_of has {session_of.size} entries for {n} items")
    return partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, ns, n


def _s2c_args(what, sigs, data32, openings, sig_format, opening_format, msghashes=None, pubkeys=None, pk_format=0, full=False):
    """shape checks shared by the sign-to-contract methods of Engine and Group: signatures (and, when full, message hashes and keys) through
    _ecdsa_args; returns (sigs, sig_off or None, msghashes, pubkeys, data32, openings, n)"""
    if opening_format not in (0, 1):
        raise ValueError(f"{what}: opening_format must be 0 (n*33 compressed) or 1 (n*64 opening objects)")
    if data32 is None or openings is None or (full and (msghashes is None or pubkeys is None)):
        raise ValueError(f"{what}: missing array")
    data32 = _u8(data32); openings = _u8(openings)
    if full:
        sigs, off, msghashes, pubkeys, n = _ecdsa_args(what, sigs, msghashes, pubkeys, sig_format, pk_format)
    else:                                            # the commitment check reads neither: the data stands in where _ecdsa_args counts 32 bytes per item
        sigs, off, _, _, n = _ecdsa_args(what, sigs, data32, openings, sig_format, opening_format)
    _need(what + " data32", data32, 32 * n); _need(what + " openings", openings, (64 if opening_format else 33) * n)
    return sigs, off, msghashes, pubkeys, data32, openings, n


_TWEAK_KEY_BYTES = {0: 32, 1: 64, 2: 33}     # serialised x-only / secp256k1_xonly_pubkey or secp256k1_pubkey object / compressed
_ELLSWIFT_OUT_BYTES = {0: 32, 1: 64, 2: 33}  # ser32(x) / secp256k1_pubkey object / compressed


def _ellswift_decode_args(what, ell64, out_format):
    """shape checks shared by the ElligatorSwift decode methods of Engine and Group; returns (ell64, n)"""
    if out_format not in _ELLSWIFT_OUT_BYTES:
        raise ValueError(f"{what}: out_format must be 0 (x only), 1 (key objects) or 2 (compressed keys)")
    if ell64 is None:
        raise ValueError(f"{what}: missing array")
    ell64 = _u8(ell64); n = ell64.size // 64
    _need(what + " ell64", ell64, 64 * n)
    return ell64, n


def _ellswift_encode_args(what, keys, key_format, rnd32):
    """returns (keys, rnd32, n)"""
    if key_format not in (1, 2):
        raise ValueError(f"{what}: key_format must be 1 (n*64 key objects) or 2 (n*33 compressed keys)")
    if keys is None or rnd32 is None:
        raise ValueError(f"{what}: missing array")
    keys = _u8(keys); rnd32 = _u8(rnd32); n = keys.size // _TWEAK_KEY_BYTES[key_format]
    _need(what + " keys", keys, _TWEAK_KEY_BYTES[key_format] * n); _need(what + " rnd32", rnd32, 32 * n)
    return keys, rnd32, n


def _tweak_check_args(what, tweaked32, parities, internal_keys, tweaks32, key_format):
    """shape checks shared by Engine.xonly_tweak_add_check_batch and Group.xonly_tweak_add_check_batch"""
    if key_format not in (0, 1):
        raise ValueError(f"{what}: key_format must be 0 (n*32 x-only keys) or 1 (n*64 key objects)")
    if tweaked32 is None or parities is None or internal_keys is None or tweaks32 is None:
        raise ValueError(f"{what}: missing array")
    tweaked32 = _u8(tweaked32); parities = _u8(parities); internal_keys = _u8(internal_keys); tweaks32 = _u8(tweaks32); n = tweaks32.size // 32
    _need(what + " tweaks32", tweaks32, 32 * n); _need(what + " tweaked32", tweaked32, 32 * n); _need(what + " parities", parities, n)
    _need(what + " internal_keys", internal_keys, _TWEAK_KEY_BYTES[key_format] * n)
    return tweaked32, parities, internal_keys, tweaks32, n


_PK_BYTES = {0: 32, 1: 64, 2: 33, 3: 65, 4: 64, 5: 64}     # include/secp256k1_zkp_amd.h: S2K_PK_*; 5 (x-only object) is an output format only


def _pk_formats(what, out_format, in_format):
    if out_format not in _PK_BYTES:
        raise ValueError(f"{what}: out_format must be 0 .. 5 (S2K_PK_*)")
    if in_format not in _PK_BYTES or in_format == 5:
        raise ValueError(f"{what}: the input format must be 0 .. 4 (S2K_PK_*; 5 is an output format)")


def _pk_tweak_mul_args(what, keys, key_format, tweaks32, out_format):
    """shape checks shared by Engine.pubkey_tweak_mul and Group.pubkey_tweak_mul"""
    _pk_formats(what, out_format, key_format)
    if keys is None or tweaks32 is None:
        raise ValueError(f"{what}: missing array")
    keys = _u8(keys); tweaks32 = _u8(tweaks32); n = tweaks32.size // 32
    _need(what + " tweaks32", tweaks32, 32 * n); _need(what + " keys", keys, _PK_BYTES[key_format] * n)
    return keys, tweaks32, n


class Engine:
    """One engine per GPU/process (owns a stream, the generator table and an HBM workspace)."""

    def __init__(self, device=0):
        self._lib = _native.load()
        self._h = self._lib.s2k_engine_create(int(device))
        if not self._h:
            raise S2KError("s2k_engine_create failed: " + _native.last_error())
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.s2k_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, ok, what):
        if not ok:
            raise S2KError(f"{what} failed: {_native.last_error()}")

    def sync(self):
        self._check(self._lib.s2k_engine_sync(self._h), "s2k_engine_sync")

    OPT_RP_INPUTS_READY = 1      # include/secp256k1_zkp_amd.h: S2K_OPT_*
    OPT_RP_SPLIT = 2
    OPT_GEN_CACHE_SLOTS = 3
    OPT_GEN_CACHE_MIN = 4
    OPT_MSM_PIPELINE = 5
    OPT_MAX_LANES = 6
    OPT_STAGE_THREADS = 7
    OPT_HALFAGG_HOST_CHAIN = 8
    OPT_SYNC_SPLIT = 9
    OPT_MSM_MAX_TERMS = 10
    OPT_GTAB_BITS = 11
    OPT_MUSIG_SUM_FANIN = 12
    OPT_S2C_FUSED = 13
    OPT_ELLSWIFT_MAX_ATTEMPTS = 14
    OPT_PUBKEY_FOLD_FANIN = 15

    def cache_generator(self, gen64):
        """Build the fixed-base table of one rangeproof generator now (s2k_engine_cache_generator)."""
        g = bytes(gen64)
        if len(g) != 64:
            raise ValueError("cache_generator: a generator is 64 bytes")
        self._check(self._lib.s2k_engine_cache_generator(self._h, g), "s2k_engine_cache_generator")

    def generator_cached(self, gen64):
        return bool(self._lib.s2k_engine_generator_cached(self._h, bytes(gen64)))

    def set_option(self, option, value):
        self._check(self._lib.s2k_engine_set_option(self._h, int(option), int(value)), "s2k_engine_set_option")

    def last_ms(self, which=0):
        return float(self._lib.s2k_engine_last_ms(self._h, which))

    def last_msm_fallback(self):
        """True if the most recent bucket MSM re-sorted exactly after a bucket region overflowed."""
        return bool(self._lib.s2k_engine_last_msm_fallback(self._h))

    def rp_handback(self):
        """(groups given to the shared-generator form, rings through the general form, rings handed back as suspect, rings handed back
        after an exceptional addition) of the most recent rangeproof call (s2k_engine_rp_handback; synchronises)."""
        out = np.zeros(4, np.uint32)
        self._check(self._lib.s2k_engine_rp_handback(self._h, _p(out)), "s2k_engine_rp_handback")
        return tuple(int(x) for x in out)

    # ---- secp256k1_ecmult (src/ecmult.h:47), batched ------------------------------------------------------
    def ecmult_batch(self, a_xy, na, ng=None, a_inf=None):
        a_xy = _u8(a_xy); n = a_xy.size // 64
        na = _u8(na); ng = None if ng is None else _u8(ng); a_inf = None if a_inf is None else _u8(a_inf)
        _need("ecmult_batch a_xy", a_xy, 64 * n); _need("ecmult_batch na", na, 32 * n)
        if ng is not None: _need("ecmult_batch ng", ng, 32 * n)
        if a_inf is not None: _need("ecmult_batch a_inf", a_inf, n)
        r = np.zeros((n, 64), np.uint8); inf = np.zeros(n, np.int32)
        self._check(self._lib.s2k_ecmult_batch(self._h, _p(r), _p(inf), _p(a_xy), _p(a_inf), _p(na), _p(ng), n), "s2k_ecmult_batch")
        return r, inf

    def ecmult_batch_dev(self, r_xy, r_inf, a_xy, na, ng=None, a_inf=None, stream=None):
        n = a_xy.numel() // 64
        self._check(self._lib.s2k_ecmult_batch_dev(self._h, stream, _dp(r_xy), _dp(r_inf), _dp(a_xy), _dp(a_inf), _dp(na), _dp(ng), n),
                    "s2k_ecmult_batch_dev")

    def ecmult2_batch(self, a_xy, na, b_xy, nb, a_inf=None, b_inf=None):
        """r[i] = na[i]*A[i] + nb[i]*B[i] (s2k_ecmult2_batch: two variable points, one chain of doublings); returns (n x 64 bytes, n flags)"""
        if a_xy is None or na is None or b_xy is None or nb is None:
            raise ValueError("ecmult2_batch: missing array")
        a_xy = _u8(a_xy); b_xy = _u8(b_xy); na = _u8(na); nb = _u8(nb); n = a_xy.size // 64
        a_inf = None if a_inf is None else _u8(a_inf); b_inf = None if b_inf is None else _u8(b_inf)
        _need("ecmult2_batch a_xy", a_xy, 64 * n); _need("ecmult2_batch b_xy", b_xy, 64 * n)
        _need("ecmult2_batch na", na, 32 * n); _need("ecmult2_batch nb", nb, 32 * n)
        if a_inf is not None: _need("ecmult2_batch a_inf", a_inf, n)
        if b_inf is not None: _need("ecmult2_batch b_inf", b_inf, n)
        r = np.zeros((n, 64), np.uint8); inf = np.zeros(n, np.int32)
        self._check(self._lib.s2k_ecmult2_batch(self._h, _p(r), _p(inf), _p(a_xy), _p(a_inf), _p(na), _p(b_xy), _p(b_inf), _p(nb), n), "s2k_ecmult2_batch")
        return r, inf

    def ecmult2_batch_dev(self, r_xy, r_inf, a_xy, na, b_xy, nb, a_inf=None, b_inf=None, stream=None):
        n = a_xy.numel() // 64
        self._check(self._lib.s2k_ecmult2_batch_dev(self._h, stream, _dp(r_xy), _dp(r_inf), _dp(a_xy), _dp(a_inf), _dp(na), _dp(b_xy), _dp(b_inf), _dp(nb), n),
                    "s2k_ecmult2_batch_dev")

    # ---- secp256k1_ecmult_multi_var (src/ecmult.h:62) ----------------------------------------------------------
    def ecmult_multi(self, sc, pt_xy, g_sc=None, pt_inf=None):
        sc = _u8(sc); pt_xy = _u8(pt_xy); n = sc.size // 32
        g_sc = None if g_sc is None else _u8(g_sc); pt_inf = None if pt_inf is None else _u8(pt_inf)
        _need("ecmult_multi sc", sc, 32 * n); _need("ecmult_multi pt_xy", pt_xy, 64 * n)
        if g_sc is not None: _need("ecmult_multi g_sc", g_sc, 32)
        if pt_inf is not None: _need("ecmult_multi pt_inf", pt_inf, n)
        r = np.zeros(64, np.uint8); inf = np.zeros(1, np.int32)
        self._check(self._lib.s2k_ecmult_multi(self._h, _p(r), _p(inf), _p(g_sc), _p(sc), _p(pt_xy), _p(pt_inf), n), "s2k_ecmult_multi")
        return r, int(inf[0])

    def ecmult_multi_dev(self, r_xy, r_inf, sc, pt_xy, g_sc=None, pt_inf=None, stream=None):
        n = sc.numel() // 32
        self._check(self._lib.s2k_ecmult_multi_dev(self._h, stream, _dp(r_xy), _dp(r_inf), _dp(g_sc), _dp(sc), _dp(pt_xy), _dp(pt_inf), n),
                    "s2k_ecmult_multi_dev")

    def ecmult_multi_many(self, sc, pt_xy, offsets, g_sc=None, pt_inf=None):
        """K independent sums in one launch chain (s2k_ecmult_multi_many): terms back to back, offsets[K + 1]; returns (K x 64 bytes, K flags)."""
        sc = _u8(sc); pt_xy = _u8(pt_xy); off = np.ascontiguousarray(offsets, dtype=np.uint64); k = off.size - 1
        n = int(off[-1]) if off.size else 0
        g_sc = None if g_sc is None else _u8(g_sc); pt_inf = None if pt_inf is None else _u8(pt_inf)
        _need("ecmult_multi_many sc", sc, 32 * n); _need("ecmult_multi_many pt_xy", pt_xy, 64 * n)
        if g_sc is not None: _need("ecmult_multi_many g_sc", g_sc, 32 * k)
        if pt_inf is not None: _need("ecmult_multi_many pt_inf", pt_inf, n)
        r = np.zeros((max(k, 0), 64), np.uint8); inf = np.zeros(max(k, 0), np.int32)
        self._check(self._lib.s2k_ecmult_multi_many(self._h, _p(r), _p(inf), _p(g_sc), _p(sc), _p(pt_xy), _p(pt_inf), _p(off), k), "s2k_ecmult_multi_many")
        return r, inf

    def ecmult_multi_many_dev(self, r_xy, r_inf, sc, pt_xy, offsets_host, g_sc=None, pt_inf=None, stream=None):
        off = np.ascontiguousarray(offsets_host, dtype=np.uint64)
        self._check(self._lib.s2k_ecmult_multi_many_dev(self._h, stream, _dp(r_xy), _dp(r_inf), _dp(g_sc), _dp(sc), _dp(pt_xy), _dp(pt_inf), _p(off), off.size - 1),
                    "s2k_ecmult_multi_many_dev")

    def ecmult_multi_partial_dev(self, r_gej28, sc, pt_xy, g_sc=None, pt_inf=None, stream=None):
        n = sc.numel() // 32
        self._check(self._lib.s2k_ecmult_multi_partial_dev(self._h, stream, _dp(r_gej28), _dp(g_sc), _dp(sc), _dp(pt_xy), _dp(pt_inf), n),
                    "s2k_ecmult_multi_partial_dev")

    def ecmult_multi_window_partial_dev(self, r_gej28, sc, pt_xy, part, parts, g_sc=None, pt_inf=None, stream=None):
        n = sc.numel() // 32
        self._check(self._lib.s2k_ecmult_multi_window_partial_dev(self._h, stream, _dp(r_gej28), _dp(g_sc), _dp(sc), _dp(pt_xy), _dp(pt_inf), n, part, parts),
                    "s2k_ecmult_multi_window_partial_dev")

    def gej_sum_dev(self, r_xy, r_inf, gej28, count, stream=None):
        self._check(self._lib.s2k_gej_sum_dev(self._h, stream, _dp(r_xy), _dp(r_inf), _dp(gej28), count), "s2k_gej_sum_dev")

    # ---- secp256k1_schnorrsig_verify (modules/schnorrsig/main_impl.h:215-261), batched -------------------------
    def schnorrsig_verify_batch(self, sigs, msgs, pubkeys, msglen=32, pk_format=0):
        sigs = _u8(sigs); msgs = _u8(msgs); pubkeys = _u8(pubkeys); n = sigs.size // 64
        _need("schnorrsig_verify_batch sigs", sigs, 64 * n); _need("schnorrsig_verify_batch msgs", msgs, msglen * n)
        _need("schnorrsig_verify_batch pubkeys", pubkeys, (64 if pk_format else 32) * n)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_schnorrsig_verify_batch(self._h, _p(res), _p(sigs), _p(msgs), msglen, _p(pubkeys), pk_format, n),
                    "secp256k1_schnorrsig_verify_batch")
        return res

    def schnorrsig_verify_batch_dev(self, results, sigs, msgs, pubkeys, msglen=32, pk_format=0, stream=None):
        n = sigs.numel() // 64
        self._check(self._lib.secp256k1_schnorrsig_verify_batch_dev(self._h, stream, _dp(results), _dp(sigs), _dp(msgs), msglen, _dp(pubkeys),
                                                                    pk_format, n), "secp256k1_schnorrsig_verify_batch_dev")

    # ---- one verdict for a whole batch of BIP-340 signatures, as a single multi-scalar multiplication (csrc/schnorr_all.h) ----
    def schnorrsig_verify_all(self, sigs, msgs, pubkeys, msglen=32, pk_format=0, locate=False, want_seed=False):
        """1 exactly when every signature of the batch verifies.  Returns the verdict; with locate=True (verdict, results) where results
        are the per-item verdicts (all ones when the verdict is 1); with want_seed=True the 32-byte seed of the coefficients is appended."""
        if pk_format not in (0, 1):
            raise ValueError("schnorrsig_verify_all: pk_format must be 0 (32-byte x-only keys) or 1 (64-byte objects)")
        if msglen < 0:
            raise ValueError("schnorrsig_verify_all: msglen must not be negative")
        if sigs is None or msgs is None or pubkeys is None:
            raise ValueError("schnorrsig_verify_all: missing array")
        sigs = _u8(sigs); msgs = _u8(msgs); pubkeys = _u8(pubkeys); n = sigs.size // 64
        _need("schnorrsig_verify_all sigs", sigs, 64 * n); _need("schnorrsig_verify_all msgs", msgs, msglen * n)
        _need("schnorrsig_verify_all pubkeys", pubkeys, (64 if pk_format else 32) * n)
        verdict = np.zeros(1, np.int32); res = np.zeros(max(n, 1), np.int32) if locate else None; seed = np.zeros(32, np.uint8) if want_seed else None
        self._check(self._lib.secp256k1_schnorrsig_verify_all(self._h, _p(verdict), _p(res), _p(seed), _p(sigs) if n else None, _p(msgs) if msgs.size else None, msglen,
                                                              _p(pubkeys) if n else None, pk_format, n), "secp256k1_schnorrsig_verify_all")
        out = (int(verdict[0]),) + ((res[:n],) if locate else ()) + ((seed.tobytes(),) if want_seed else ())
        return out[0] if len(out) == 1 else out

    def schnorrsig_verify_all_dev(self, verdict, sigs, msgs, pubkeys, msglen=32, pk_format=0, seed_out=None, n=None, stream=None):
        """every array in HBM (torch tensors): verdict int32[1], seed_out uint8[32] or None; nothing is read back"""
        if pk_format not in (0, 1):
            raise ValueError("schnorrsig_verify_all_dev: pk_format must be 0 or 1")
        if n is None:
            n = sigs.numel() // 64
        if verdict is None or verdict.numel() < 1 or (seed_out is not None and seed_out.numel() < 32):
            raise ValueError("schnorrsig_verify_all_dev: verdict needs one int32 and seed_out 32 bytes")
        if n and (sigs.numel() < 64 * n or pubkeys.numel() < (64 if pk_format else 32) * n or (msglen and msgs.numel() < msglen * n)):
            raise ValueError("schnorrsig_verify_all_dev: fewer signature / message / key bytes than n needs")
        self._check(self._lib.secp256k1_schnorrsig_verify_all_dev(self._h, stream, _dp(verdict), _dp(seed_out), _dp(sigs) if n else None, _dp(msgs) if n and msglen else None,
                                                                  msglen, _dp(pubkeys) if n else None, pk_format, n), "secp256k1_schnorrsig_verify_all_dev")

    def schnorr_all_last_split_ms(self):
        """[lift + item hashes, tree + seed, coefficients + scalar sum, MSM] of the most recent verify_all call, in ms (after sync())"""
        out = np.full(4, -1.0, np.float32)
        self._check(self._lib.s2k_schnorr_all_last_split_ms(self._h, _p(out)), "s2k_schnorr_all_last_split_ms")
        return [float(x) for x in out]

    # ---- secp256k1_ecdsa_verify (secp256k1.c:498-512, ecdsa_impl.h:195-272) and secp256k1_ecdsa_recover (modules/recovery/main_impl.h:87-157), batched ----
    def ecdsa_verify_batch(self, sigs, msghashes, pubkeys, sig_format=0, pk_format=0):
        """sig_format 0: n*64 compact, 1: n*64 secp256k1_ecdsa_signature objects, 2: DER -- a list of bytes (packed here) or the tuple (data, offsets[n+1]);
        pk_format 0: n*33 compressed, 1: n*64 secp256k1_pubkey objects, 2: n*65 uncompressed / hybrid"""
        sigs, off, msghashes, pubkeys, n = _ecdsa_args("ecdsa_verify_batch", sigs, msghashes, pubkeys, sig_format, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_verify_batch(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(msghashes), _p(pubkeys), pk_format, n),
                    "secp256k1_ecdsa_verify_batch")
        return res

    def ecdsa_verify_batch_dev(self, results, sigs, msghashes, pubkeys, sig_format=0, pk_format=0, sig_off=None, n=None, stream=None):
        """every array in HBM (torch tensors; sig_off: int64 / uint64 offsets[n+1], DER only)"""
        if sig_format == 2 and sig_off is None:
            raise ValueError("ecdsa_verify_batch_dev: DER signatures need sig_off")
        if n is None:
            n = sig_off.numel() - 1 if sig_format == 2 else sigs.numel() // 64
        self._check(self._lib.secp256k1_ecdsa_verify_batch_dev(self._h, stream, _dp(results), _dp(sigs), _dp(sig_off) if sig_format == 2 else None, sig_format,
                                                               _dp(msghashes), _dp(pubkeys), pk_format, n), "secp256k1_ecdsa_verify_batch_dev")

    def ecdsa_recover_batch(self, sigs64, recids, msghashes):
        """-> (results[n], pubkeys64[n, 64]): secp256k1_pubkey objects (pk_format 1 of ecdsa_verify_batch), zero where results[i] == 0"""
        sigs64 = _u8(sigs64); recids = _u8(recids); msghashes = _u8(msghashes); n = sigs64.size // 64
        _need("ecdsa_recover_batch sigs64", sigs64, 64 * n); _need("ecdsa_recover_batch recids", recids, n); _need("ecdsa_recover_batch msghashes", msghashes, 32 * n)
        res = np.zeros(n, np.int32); pk = np.zeros((n, 64), np.uint8)
        self._check(self._lib.secp256k1_ecdsa_recover_batch(self._h, _p(res), _p(pk), _p(sigs64), _p(recids), _p(msghashes), n), "secp256k1_ecdsa_recover_batch")
        return res, pk

    def ecdsa_recover_batch_dev(self, results, pubkeys_out64, sigs64, recids, msghashes, n=None, stream=None):
        n = sigs64.numel() // 64 if n is None else n
        self._check(self._lib.secp256k1_ecdsa_recover_batch_dev(self._h, stream, _dp(results), _dp(pubkeys_out64), _dp(sigs64), _dp(recids), _dp(msghashes), n),
                    "secp256k1_ecdsa_recover_batch_dev")

    # ---- secp256k1_ecdsa_adaptor_verify (modules/ecdsa_adaptor/main_impl.h:236-282), batched ----
    def ecdsa_adaptor_verify_batch(self, adaptor_sigs, pubkeys, msgs32, enckeys, pk_format=0):
        """adaptor_sigs n*162; pubkeys and enckeys in one pk_format (0: n*33 compressed, 1: n*64 secp256k1_pubkey objects, 2: n*65); msgs32 n*32"""
        adaptor_sigs, pubkeys, msgs32, enckeys, n = _adaptor_args("ecdsa_adaptor_verify_batch", adaptor_sigs, pubkeys, msgs32, enckeys, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_adaptor_verify_batch(self._h, _p(res), _p(adaptor_sigs), _p(pubkeys), _p(msgs32), _p(enckeys), pk_format, n),
                    "secp256k1_ecdsa_adaptor_verify_batch")
        return res

    def ecdsa_adaptor_verify_batch_dev(self, results, adaptor_sigs, pubkeys, msgs32, enckeys, pk_format=0, n=None, stream=None):
        """every array in HBM (torch tensors)"""
        n = adaptor_sigs.numel() // 162 if n is None else n
        self._check(self._lib.secp256k1_ecdsa_adaptor_verify_batch_dev(self._h, stream, _dp(results), _dp(adaptor_sigs), _dp(pubkeys), _dp(msgs32), _dp(enckeys),
                                                                       pk_format, n), "secp256k1_ecdsa_adaptor_verify_batch_dev")

    # ---- secp256k1_ecdsa_s2c_verify_commit, secp256k1_anti_exfil_host_verify and secp256k1_ecdsa_anti_exfil_host_commit (modules/ecdsa_s2c/main_impl.h:88-188), batched ----
    def ecdsa_s2c_verify_commit_batch(self, sigs, data32, openings, sig_format=0, opening_format=0):
        """sigs and sig_format as ecdsa_verify_batch; data32 n*32; openings: opening_format 0: n*33 compressed, 1: n*64 secp256k1_ecdsa_s2c_opening objects"""
        sigs, off, _, _, data32, openings, n = _s2c_args("ecdsa_s2c_verify_commit_batch", sigs, data32, openings, sig_format, opening_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_s2c_verify_commit_batch(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(data32), _p(openings), opening_format, n),
                    "secp256k1_ecdsa_s2c_verify_commit_batch")
        return res

    def ecdsa_s2c_verify_commit_batch_dev(self, results, sigs, data32, openings, sig_format=0, opening_format=0, sig_off=None, n=None, stream=None):
        """every array in HBM (torch tensors; sig_off: int64 / uint64 offsets[n+1], DER only)"""
        if sig_format == 2 and sig_off is None:
            raise ValueError("ecdsa_s2c_verify_commit_batch_dev: DER signatures need sig_off")
        if n is None:
            n = sig_off.numel() - 1 if sig_format == 2 else sigs.numel() // 64
        self._check(self._lib.secp256k1_ecdsa_s2c_verify_commit_batch_dev(self._h, stream, _dp(results), _dp(sigs), _dp(sig_off) if sig_format == 2 else None, sig_format,
                                                                          _dp(data32), _dp(openings), opening_format, n), "secp256k1_ecdsa_s2c_verify_commit_batch_dev")

    def anti_exfil_host_verify_batch(self, sigs, msghashes, pubkeys, host_data32, openings, sig_format=0, pk_format=0, opening_format=0):
        """sigs, msghashes, pubkeys, sig_format and pk_format as ecdsa_verify_batch; host_data32 n*32; openings as ecdsa_s2c_verify_commit_batch"""
        sigs, off, msghashes, pubkeys, host_data32, openings, n = _s2c_args("anti_exfil_host_verify_batch", sigs, host_data32, openings, sig_format, opening_format,
                                                                            msghashes, pubkeys, pk_format, full=True)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_anti_exfil_host_verify_batch(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(msghashes), _p(pubkeys), pk_format,
                                                                     _p(host_data32), _p(openings), opening_format, n), "secp256k1_anti_exfil_host_verify_batch")
        return res

    def anti_exfil_host_verify_batch_dev(self, results, sigs, msghashes, pubkeys, host_data32, openings, sig_format=0, pk_format=0, opening_format=0, sig_off=None,
                                         n=None, stream=None):
        """every array in HBM (torch tensors; sig_off: int64 / uint64 offsets[n+1], DER only)"""
        if sig_format == 2 and sig_off is None:
            raise ValueError("anti_exfil_host_verify_batch_dev: DER signatures need sig_off")
        if n is None:
            n = sig_off.numel() - 1 if sig_format == 2 else sigs.numel() // 64
        self._check(self._lib.secp256k1_anti_exfil_host_verify_batch_dev(self._h, stream, _dp(results), _dp(sigs), _dp(sig_off) if sig_format == 2 else None, sig_format,
                                                                         _dp(msghashes), _dp(pubkeys), pk_format, _dp(host_data32), _dp(openings), opening_format, n),
                    "secp256k1_anti_exfil_host_verify_batch_dev")

    def anti_exfil_host_commit_batch(self, rand32):
        """-> commitments[n, 32]: what secp256k1_ecdsa_anti_exfil_host_commit writes for each 32-byte input"""
        if rand32 is None:
            raise ValueError("anti_exfil_host_commit_batch: missing array")
        rand32 = _u8(rand32); n = rand32.size // 32
        _need("anti_exfil_host_commit_batch rand32", rand32, 32 * n)
        out = np.zeros((n, 32), np.uint8)
        self._check(self._lib.secp256k1_ecdsa_anti_exfil_host_commit_batch(self._h, _p(out), _p(rand32), n), "secp256k1_ecdsa_anti_exfil_host_commit_batch")
        return out

    def anti_exfil_host_commit_batch_dev(self, commitments_out32, rand32, n=None, stream=None):
        n = rand32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_ecdsa_anti_exfil_host_commit_batch_dev(self._h, stream, _dp(commitments_out32), _dp(rand32), n),
                    "secp256k1_ecdsa_anti_exfil_host_commit_batch_dev")

    # ---- secp256k1_musig_partial_sig_verify and secp256k1_musig_nonce_process (modules/musig/session_impl.h:716-777, :588-638), batched ----
    def musig_partial_sig_verify(self, partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of=None, sig_format=0, nonce_format=0, pk_format=0):
        """partial_sigs n*32 serialised or n*36 objects; pubnonces n*66 serialised or n*132 objects; pubkeys in pk_format (0: n*33, 1: n*64
        objects, 2: n*65); keyagg_caches n_sessions*197 and sessions n_sessions*133, one pair per signing session; session_of: the pair of
        each share (uint32), or None when there is one pair per share.  An index >= n_sessions is an error."""
        partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, ns, n = _musig_verify_args(
            "musig_partial_sig_verify", partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, sig_format, nonce_format, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_musig_partial_sig_verify_batch(self._h, _p(res), _p(partial_sigs), sig_format, _p(pubnonces), nonce_format, _p(pubkeys), pk_format,
                                                                       _p(keyagg_caches), _p(sessions), ns, _p(session_of), n), "secp256k1_musig_partial_sig_verify_batch")
        return res

    def musig_partial_sig_verify_dev(self, results, partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, n_sessions, session_of=None, sig_format=0, nonce_format=0,
                                     pk_format=0, n=None, stream=None):
        """every array in HBM (torch tensors), session_of (int32 / uint32 storage) included; a share whose index is >= n_sessions gets 0"""
        n = partial_sigs.numel() // (36 if sig_format else 32) if n is None else n
        self._check(self._lib.secp256k1_musig_partial_sig_verify_batch_dev(self._h, stream, _dp(results), _dp(partial_sigs), sig_format, _dp(pubnonces), nonce_format,
                                                                           _dp(pubkeys), pk_format, _dp(keyagg_caches), _dp(sessions), n_sessions, _dp(session_of), n),
                    "secp256k1_musig_partial_sig_verify_batch_dev")

    def musig_nonce_process(self, aggnonces, msgs32, keyagg_caches, adaptors=None, nonce_format=0):
        """aggnonces n*66 serialised or n*132 objects; msgs32 n*32; keyagg_caches n*197; adaptors None or n*64 secp256k1_pubkey objects.
        Returns (verdicts, n*133 session bytes); a session whose verdict is 0 is all zero."""
        if nonce_format not in (0, 1):
            raise ValueError("musig_nonce_process: nonce_format must be 0 or 1")
        if aggnonces is None or msgs32 is None or keyagg_caches is None:
            raise ValueError("musig_nonce_process: missing array")
        aggnonces = _u8(aggnonces); msgs32 = _u8(msgs32); keyagg_caches = _u8(keyagg_caches); n = msgs32.size // 32
        _need("musig_nonce_process aggnonces", aggnonces, (132 if nonce_format else 66) * n); _need("musig_nonce_process msgs32", msgs32, 32 * n)
        _need("musig_nonce_process keyagg_caches", keyagg_caches, 197 * n)
        if adaptors is not None:
            adaptors = _u8(adaptors); _need("musig_nonce_process adaptors", adaptors, 64 * n)
        res = np.zeros(n, np.int32); out = np.zeros(133 * n, np.uint8)
        self._check(self._lib.secp256k1_musig_nonce_process_batch(self._h, _p(res), _p(out), _p(aggnonces), nonce_format, _p(msgs32), _p(keyagg_caches), _p(adaptors), n),
                    "secp256k1_musig_nonce_process_batch")
        return res, out

    def musig_nonce_process_dev(self, results, sessions_out, aggnonces, msgs32, keyagg_caches, adaptors=None, nonce_format=0, n=None, stream=None):
        """every array in HBM (torch tensors); sessions_out n*133 feeds musig_partial_sig_verify_dev on the same stream"""
        n = msgs32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_musig_nonce_process_batch_dev(self._h, stream, _dp(results), _dp(sessions_out), _dp(aggnonces), nonce_format, _dp(msgs32),
                                                                      _dp(keyagg_caches), _dp(adaptors), n), "secp256k1_musig_nonce_process_batch_dev")

    # ---- secp256k1_musig_pubkey_agg, the cache tweaks, secp256k1_musig_nonce_agg and secp256k1_musig_partial_sig_agg (keyagg_impl.h:156-273, session_impl.h:512-531, :779-805), batched ----
    @staticmethod
    def _musig_off(what, off, item_bytes, data):
        """offsets (n + 1 entries, counted in items) as a uint64 host array, checked against the data array"""
        if off is None:
            raise ValueError(f"{what}: missing offsets")
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError(f"{what}: offsets need n + 1 entries")
        o = off.astype(np.int64)
        if int(o[0]) != 0 or (np.diff(o) < 0).any():
            raise ValueError(f"{what}: offsets must start at 0 and never decrease")
        if data is not None:
            _need(what, data, item_bytes * int(o[-1]))
        return off

    def musig_pubkey_agg(self, pubkeys, set_off, pk_format=0, want_agg_pk=True):
        """pubkeys: the keys of all sets, concatenated (pk_format 0: 33 bytes each, 1: 64-byte objects, 2: 65 bytes); set k owns keys
        [set_off[k], set_off[k+1]).  Returns (verdicts, n_sets*197 cache bytes, n_sets*64 x-only key objects or None); the outputs of a
        refused set (empty, a key that does not parse, an aggregate at infinity) are all zero."""
        if pk_format not in _ECDSA_PK_BYTES:
            raise ValueError("musig_pubkey_agg: pk_format must be 0, 1 or 2")
        if pubkeys is None:
            raise ValueError("musig_pubkey_agg: missing array")
        pubkeys = _u8(pubkeys)
        set_off = self._musig_off("musig_pubkey_agg", set_off, _ECDSA_PK_BYTES[pk_format], pubkeys)
        n = set_off.size - 1
        res = np.zeros(n, np.int32); caches = np.zeros(197 * n, np.uint8); agg = np.zeros(64 * n, np.uint8) if want_agg_pk else None
        self._check(self._lib.secp256k1_musig_pubkey_agg_batch(self._h, _p(res), _p(caches), _p(agg), _p(pubkeys), pk_format, _p(set_off), n), "secp256k1_musig_pubkey_agg_batch")
        return res, caches, agg

    def musig_pubkey_agg_dev(self, results, caches_out, agg_pks_out, pubkeys, set_off, pk_format=0, stream=None):
        """byte arrays in HBM (torch tensors; agg_pks_out may be None); set_off is a HOST array of n_sets + 1 key counts, read before the call returns"""
        set_off = self._musig_off("musig_pubkey_agg_dev", set_off, 0, None)
        self._check(self._lib.secp256k1_musig_pubkey_agg_batch_dev(self._h, stream, _dp(results), _dp(caches_out), _dp(agg_pks_out), _dp(pubkeys), pk_format, _p(set_off),
                                                                   set_off.size - 1), "secp256k1_musig_pubkey_agg_batch_dev")

    def musig_pubkey_tweak_add(self, keyagg_caches, tweaks32, xonly=None, want_pubkeys=True):
        """keyagg_caches n*197; tweaks32 n*32; xonly None (all plain tweaks) or one byte per item (1: x-only, 0: plain; anything else is
        refused).  Returns (verdicts, n*197 new cache bytes, n*64 secp256k1_pubkey objects or None); a refused item's outputs are all zero."""
        if keyagg_caches is None or tweaks32 is None:
            raise ValueError("musig_pubkey_tweak_add: missing array")
        keyagg_caches = _u8(keyagg_caches); tweaks32 = _u8(tweaks32); n = tweaks32.size // 32
        _need("musig_pubkey_tweak_add keyagg_caches", keyagg_caches, 197 * n); _need("musig_pubkey_tweak_add tweaks32", tweaks32, 32 * n)
        if xonly is not None:
            xonly = _u8(xonly); _need("musig_pubkey_tweak_add xonly", xonly, n)
        res = np.zeros(n, np.int32); out = np.zeros(197 * n, np.uint8); pks = np.zeros(64 * n, np.uint8) if want_pubkeys else None
        self._check(self._lib.secp256k1_musig_pubkey_tweak_add_batch(self._h, _p(res), _p(out), _p(pks), _p(keyagg_caches), _p(tweaks32), _p(xonly), n),
                    "secp256k1_musig_pubkey_tweak_add_batch")
        return res, out, pks

    def musig_pubkey_tweak_add_dev(self, results, caches_out, pubkeys_out, caches_in, tweaks32, xonly=None, n=None, stream=None):
        """every array in HBM (torch tensors); caches_out may be caches_in; pubkeys_out and xonly may be None"""
        n = tweaks32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_musig_pubkey_tweak_add_batch_dev(self._h, stream, _dp(results), _dp(caches_out), _dp(pubkeys_out), _dp(caches_in), _dp(tweaks32),
                                                                         _dp(xonly), n), "secp256k1_musig_pubkey_tweak_add_batch_dev")

    def musig_nonce_agg(self, pubnonces, nonce_off, nonce_format=0, out_format=0):
        """pubnonces: 66 bytes serialised or 132-byte objects each, all sessions concatenated; session k owns [nonce_off[k], nonce_off[k+1]).
        Returns (verdicts, aggregate nonces: 66 bytes serialised or 132-byte objects each, all zero where the verdict is 0)."""
        if nonce_format not in (0, 1) or out_format not in (0, 1):
            raise ValueError("musig_nonce_agg: nonce_format and out_format must be 0 or 1")
        if pubnonces is None:
            raise ValueError("musig_nonce_agg: missing array")
        pubnonces = _u8(pubnonces)
        nonce_off = self._musig_off("musig_nonce_agg", nonce_off, 132 if nonce_format else 66, pubnonces)
        n = nonce_off.size - 1
        res = np.zeros(n, np.int32); out = np.zeros((132 if out_format else 66) * n, np.uint8)
        self._check(self._lib.secp256k1_musig_nonce_agg_batch(self._h, _p(res), _p(out), out_format, _p(pubnonces), nonce_format, _p(nonce_off), n), "secp256k1_musig_nonce_agg_batch")
        return res, out

    def musig_nonce_agg_dev(self, results, aggnonces_out, pubnonces, nonce_off, nonce_format=0, out_format=0, stream=None):
        """byte arrays in HBM (torch tensors); nonce_off is a HOST array; aggnonces_out feeds musig_nonce_process_dev on the same stream"""
        nonce_off = self._musig_off("musig_nonce_agg_dev", nonce_off, 0, None)
        self._check(self._lib.secp256k1_musig_nonce_agg_batch_dev(self._h, stream, _dp(results), _dp(aggnonces_out), out_format, _dp(pubnonces), nonce_format, _p(nonce_off),
                                                                  nonce_off.size - 1), "secp256k1_musig_nonce_agg_batch_dev")

    def musig_partial_sig_agg(self, sessions, partial_sigs, sig_off, sig_format=0):
        """sessions n*133; partial_sigs 32 bytes serialised or 36-byte objects each, all sessions concatenated; session k owns
        [sig_off[k], sig_off[k+1]).  Returns (verdicts, n*64 BIP-340 signatures, all zero where the verdict is 0)."""
        if sig_format not in (0, 1):
            raise ValueError("musig_partial_sig_agg: sig_format must be 0 or 1")
        if sessions is None or partial_sigs is None:
            raise ValueError("musig_partial_sig_agg: missing array")
        sessions = _u8(sessions); partial_sigs = _u8(partial_sigs)
        sig_off = self._musig_off("musig_partial_sig_agg", sig_off, 36 if sig_format else 32, partial_sigs)
        n = sig_off.size - 1
        _need("musig_partial_sig_agg sessions", sessions, 133 * n)
        res = np.zeros(n, np.int32); out = np.zeros(64 * n, np.uint8)
        self._check(self._lib.secp256k1_musig_partial_sig_agg_batch(self._h, _p(res), _p(out), _p(sessions), _p(partial_sigs), sig_format, _p(sig_off), n),
                    "secp256k1_musig_partial_sig_agg_batch")
        return res, out

    def musig_partial_sig_agg_dev(self, results, sigs64_out, sessions, partial_sigs, sig_off, sig_format=0, stream=None):
        """byte arrays in HBM (torch tensors); sig_off is a HOST array; sigs64_out are BIP-340 signatures"""
        sig_off = self._musig_off("musig_partial_sig_agg_dev", sig_off, 0, None)
        self._check(self._lib.secp256k1_musig_partial_sig_agg_batch_dev(self._h, stream, _dp(results), _dp(sigs64_out), _dp(sessions), _dp(partial_sigs), sig_format, _p(sig_off),
                                                                        sig_off.size - 1), "secp256k1_musig_partial_sig_agg_batch_dev")

    # ---- secp256k1_xonly_pubkey_tweak_add_check / _tweak_add (modules/extrakeys/main_impl.h:118-154) and secp256k1_ec_pubkey_tweak_add (secp256k1.c:766-790), batched ----
    def xonly_tweak_add_check_batch(self, tweaked32, parities, internal_keys, tweaks32, key_format=0):
        """key_format 0: n*32 serialised x-only internal keys, 1: n*64 secp256k1_xonly_pubkey objects; parities: one byte per item"""
        tweaked32, parities, internal_keys, tweaks32, n = _tweak_check_args("xonly_tweak_add_check_batch", tweaked32, parities, internal_keys, tweaks32, key_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_xonly_pubkey_tweak_add_check_batch(self._h, _p(res), _p(tweaked32), _p(parities), _p(internal_keys), key_format, _p(tweaks32), n),
                    "secp256k1_xonly_pubkey_tweak_add_check_batch")
        return res

    def xonly_tweak_add_check_batch_dev(self, results, tweaked32, parities, internal_keys, tweaks32, key_format=0, n=None, stream=None):
        """every array in HBM (torch tensors)"""
        n = tweaks32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_xonly_pubkey_tweak_add_check_batch_dev(self._h, stream, _dp(results), _dp(tweaked32), _dp(parities), _dp(internal_keys), key_format,
                                                                               _dp(tweaks32), n), "secp256k1_xonly_pubkey_tweak_add_check_batch_dev")

    def pubkey_tweak_add_batch(self, keys, tweaks32, key_format=1):
        """key_format 0: n*32 x-only keys, 1: n*64 key objects, 2: n*33 compressed keys
        -> (results[n], pubkeys64[n, 64]): secp256k1_pubkey objects (key_format 1 reads them), zero where results[i] == 0"""
        if key_format not in _TWEAK_KEY_BYTES:
            raise ValueError("pubkey_tweak_add_batch: key_format must be 0, 1 or 2")
        if keys is None or tweaks32 is None:
            raise ValueError("pubkey_tweak_add_batch: missing array")
        keys = _u8(keys); tweaks32 = _u8(tweaks32); n = tweaks32.size // 32
        _need("pubkey_tweak_add_batch tweaks32", tweaks32, 32 * n); _need("pubkey_tweak_add_batch keys", keys, _TWEAK_KEY_BYTES[key_format] * n)
        res = np.zeros(n, np.int32); pk = np.zeros((n, 64), np.uint8)
        self._check(self._lib.secp256k1_pubkey_tweak_add_batch(self._h, _p(res), _p(pk), _p(keys), key_format, _p(tweaks32), n), "secp256k1_pubkey_tweak_add_batch")
        return res, pk

    def pubkey_tweak_add_batch_dev(self, results, pubkeys_out64, keys, tweaks32, key_format=1, n=None, stream=None):
        n = tweaks32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_pubkey_tweak_add_batch_dev(self._h, stream, _dp(results), _dp(pubkeys_out64), _dp(keys), key_format, _dp(tweaks32), n),
                    "secp256k1_pubkey_tweak_add_batch_dev")

    # ---- the public-key group of include/secp256k1.h and secp256k1_extrakeys.h: conversion, negation, tweak-mul, combine (csrc/pubkey.h), batched ----
    def _pk_convert(self, what, keys, in_format, out_format):
        _pk_formats(what, out_format, in_format)
        if keys is None:
            raise ValueError(f"{what}: missing array")
        keys = _u8(keys); n = keys.size // _PK_BYTES[in_format]
        _need(what + " keys", keys, _PK_BYTES[in_format] * n)
        res = np.zeros(n, np.int32); out = np.zeros((n, _PK_BYTES[out_format]), np.uint8); par = np.zeros(n, np.uint8)
        self._check(getattr(self._lib, what)(self._h, _p(res), _p(out), out_format, _p(par), _p(keys), in_format, n), what)
        return res, out, par

    def pubkey_convert(self, keys, in_format, out_format):
        """keys: n keys in in_format (S2K_PK_*: 0 x-only 32 bytes, 1 object 64, 2 compressed 33, 3 uncompressed / hybrid 65, 4 x | y 64)
        -> (results[n], out[n, bytes of out_format], parities[n]); out_format also 5: the object with y made even.  A refused key's output is zero."""
        return self._pk_convert("secp256k1_ec_pubkey_convert_batch", keys, in_format, out_format)

    def pubkey_convert_dev(self, results, out, keys, in_format, out_format, parities_out=None, n=None, stream=None):
        """every array in HBM (torch tensors); parities_out may be None"""
        _pk_formats("pubkey_convert_dev", out_format, in_format)
        n = keys.numel() // _PK_BYTES[in_format] if n is None else n
        self._check(self._lib.secp256k1_ec_pubkey_convert_batch_dev(self._h, stream, _dp(results), _dp(out), out_format, _dp(parities_out), _dp(keys), in_format, n),
                    "secp256k1_ec_pubkey_convert_batch_dev")

    def pubkey_negate(self, keys, in_format, out_format):
        """as pubkey_convert, with every key negated (secp256k1_ec_pubkey_negate)"""
        return self._pk_convert("secp256k1_ec_pubkey_negate_batch", keys, in_format, out_format)

    def pubkey_negate_dev(self, results, out, keys, in_format, out_format, parities_out=None, n=None, stream=None):
        _pk_formats("pubkey_negate_dev", out_format, in_format)
        n = keys.numel() // _PK_BYTES[in_format] if n is None else n
        self._check(self._lib.secp256k1_ec_pubkey_negate_batch_dev(self._h, stream, _dp(results), _dp(out), out_format, _dp(parities_out), _dp(keys), in_format, n),
                    "secp256k1_ec_pubkey_negate_batch_dev")

    def pubkey_tweak_mul(self, keys, tweaks32, key_format=1, out_format=1):
        """results[i] = secp256k1_ec_pubkey_tweak_mul(key_i, tweak32_i) -> (results[n], out[n, bytes of out_format], parities[n]);
        0 and zero bytes for a tweak >= the group order, a tweak of 0 and a key that does not load"""
        keys, tweaks32, n = _pk_tweak_mul_args("pubkey_tweak_mul", keys, key_format, tweaks32, out_format)
        res = np.zeros(n, np.int32); out = np.zeros((n, _PK_BYTES[out_format]), np.uint8); par = np.zeros(n, np.uint8)
        self._check(self._lib.secp256k1_ec_pubkey_tweak_mul_batch(self._h, _p(res), _p(out), out_format, _p(par), _p(keys), key_format, _p(tweaks32), n),
                    "secp256k1_ec_pubkey_tweak_mul_batch")
        return res, out, par

    def pubkey_tweak_mul_dev(self, results, out, keys, tweaks32, key_format=1, out_format=1, parities_out=None, n=None, stream=None):
        _pk_formats("pubkey_tweak_mul_dev", out_format, key_format)
        n = tweaks32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_ec_pubkey_tweak_mul_batch_dev(self._h, stream, _dp(results), _dp(out), out_format, _dp(parities_out), _dp(keys), key_format,
                                                                      _dp(tweaks32), n), "secp256k1_ec_pubkey_tweak_mul_batch_dev")

    def pubkey_combine(self, keys, key_off, key_format=1, out_format=1):
        """keys: the keys of all sets, concatenated; set k owns keys [key_off[k], key_off[k+1]) (n_sets + 1 entries, starting at 0, never
        decreasing).  -> (results[n_sets], out[n_sets, bytes of out_format], parities[n_sets]): secp256k1_ec_pubkey_combine per set; 0 and
        zero bytes for an empty set, a set with a key that does not load and a sum at infinity.  Formats 1 and 4 are the fast path."""
        _pk_formats("pubkey_combine", out_format, key_format)
        if keys is None:
            raise ValueError("pubkey_combine: missing array")
        keys = _u8(keys)
        key_off = self._musig_off("pubkey_combine", key_off, _PK_BYTES[key_format], keys)
        n = key_off.size - 1
        res = np.zeros(n, np.int32); out = np.zeros((n, _PK_BYTES[out_format]), np.uint8); par = np.zeros(n, np.uint8)
        self._check(self._lib.secp256k1_ec_pubkey_combine_batch(self._h, _p(res), _p(out), out_format, _p(par), _p(keys), key_format, _p(key_off), n),
                    "secp256k1_ec_pubkey_combine_batch")
        return res, out, par

    def pubkey_combine_dev(self, results, out, keys, key_off, key_format=1, out_format=1, parities_out=None, stream=None):
        """byte arrays in HBM (torch tensors); key_off is a HOST array of n_sets + 1 key counts, read before the call returns"""
        _pk_formats("pubkey_combine_dev", out_format, key_format)
        key_off = self._musig_off("pubkey_combine_dev", key_off, 0, None)
        self._check(self._lib.secp256k1_ec_pubkey_combine_batch_dev(self._h, stream, _dp(results), _dp(out), out_format, _dp(parities_out), _dp(keys), key_format, _p(key_off),
                                                                    key_off.size - 1), "secp256k1_ec_pubkey_combine_batch_dev")

    # ---- SHA-256, double SHA-256 and secp256k1_tagged_sha256 (secp256k1.c:869-881) of one message per lane; BIP-340 with a length per item ----
    @staticmethod
    def _msg_items(what, msgs, msg_off, msglen, n):
        """host arrays -> (msgs, msg_off or None, msglen, n).  Exactly one of msg_off / msglen; decreasing offsets are left to the library."""
        if (msg_off is None) == (msglen is None):
            raise ValueError(f"{what}: give exactly one of msg_off and msglen")
        if msgs is None:
            raise ValueError(f"{what}: missing array")
        msgs = _u8(msgs)
        if msg_off is not None:
            msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
            if msg_off.size == 0:
                raise S2KError(f"{what}: msg_off is empty (it has n + 1 entries)")
            if int(msg_off.max()) > msgs.size:
                raise ValueError(f"{what}: msg_off points behind the data ({msgs.size} bytes)")
            return msgs, msg_off, 0, msg_off.size - 1
        msglen = int(msglen)
        if msglen < 0:
            raise ValueError(f"{what}: msglen must not be negative")
        if n is None:
            if msglen == 0:
                raise ValueError(f"{what}: msglen 0 needs n")
            n = msgs.size // msglen
        _need(what + " msgs", msgs, msglen * n)
        return msgs, None, msglen, n

    @staticmethod
    def _msg_items_dev(what, msg_off, msglen, msgs, n):
        if (msg_off is None) == (msglen is None):
            raise ValueError(f"{what}: give exactly one of msg_off and msglen")
        if msg_off is not None:
            if msg_off.numel() == 0:
                raise S2KError(f"{what}: msg_off is empty (it has n + 1 entries)")
            return 0, msg_off.numel() - 1 if n is None else n
        msglen = int(msglen)
        if msglen < 0 or (n is None and msglen == 0):
            raise ValueError(f"{what}: msglen must not be negative, and msglen 0 needs n")
        return msglen, msgs.numel() // msglen if n is None else n

    def sha256_batch(self, msgs, msg_off=None, msglen=None, rounds=1, n=None):
        """-> digests[n, 32]: SHA256 (rounds 1) or SHA256 of SHA256 (rounds 2) of every item.  msglen: n items of msglen bytes back to back;
        msg_off: uint64[n+1], item i is msgs[msg_off[i] .. msg_off[i+1]).  Exactly one of the two."""
        msgs, msg_off, msglen, n = self._msg_items("sha256_batch", msgs, msg_off, msglen, n)
        out = np.zeros((n, 32), np.uint8)
        pad = msgs if msgs.size else np.zeros(1, np.uint8)
        self._check(self._lib.s2k_sha256_batch(self._h, _p(out), _p(pad), _p(msg_off), msglen, int(rounds), n), "s2k_sha256_batch")
        return out

    def sha256_batch_dev(self, out32, msgs, msg_off=None, msglen=None, rounds=1, n=None, stream=None):
        """every array in HBM (torch tensors; msg_off: int64 / uint64 offsets[n+1]).  An item whose offsets decrease gets 32 zero bytes."""
        msglen, n = self._msg_items_dev("sha256_batch_dev", msg_off, msglen, msgs, n)
        self._check(self._lib.s2k_sha256_batch_dev(self._h, stream, _dp(out32), _dp(msgs), _dp(msg_off), msglen, int(rounds), n), "s2k_sha256_batch_dev")

    def tagged_sha256_batch(self, tag, msgs, msg_off=None, msglen=None, n=None):
        """-> digests[n, 32]: secp256k1_tagged_sha256(tag, item) of every item; tag: bytes.  Items as in sha256_batch."""
        if tag is None:
            raise ValueError("tagged_sha256_batch: missing tag")
        tag = bytes(tag)
        msgs, msg_off, msglen, n = self._msg_items("tagged_sha256_batch", msgs, msg_off, msglen, n)
        out = np.zeros((n, 32), np.uint8)
        pad = msgs if msgs.size else np.zeros(1, np.uint8)
        self._check(self._lib.secp256k1_tagged_sha256_batch(self._h, _p(out), tag, len(tag), _p(pad), _p(msg_off), msglen, n), "secp256k1_tagged_sha256_batch")
        return out

    def tagged_sha256_batch_dev(self, out32, tag, msgs, msg_off=None, msglen=None, n=None, stream=None):
        """tag: bytes on the host; every array in HBM (torch tensors)"""
        if tag is None:
            raise ValueError("tagged_sha256_batch_dev: missing tag")
        tag = bytes(tag)
        msglen, n = self._msg_items_dev("tagged_sha256_batch_dev", msg_off, msglen, msgs, n)
        self._check(self._lib.secp256k1_tagged_sha256_batch_dev(self._h, stream, _dp(out32), tag, len(tag), _dp(msgs), _dp(msg_off), msglen, n),
                    "secp256k1_tagged_sha256_batch_dev")

    def schnorrsig_verify_batch_var(self, sigs, msgs, msg_off, pubkeys, pk_format=0):
        """results[i] = secp256k1_schnorrsig_verify(sig_i, msgs[msg_off[i] .. msg_off[i+1]), pubkey_i): a message length per item"""
        if pk_format not in (0, 1):
            raise ValueError("schnorrsig_verify_batch_var: pk_format must be 0 (32-byte x-only keys) or 1 (64-byte objects)")
        if msg_off is None or sigs is None or pubkeys is None:
            raise ValueError("schnorrsig_verify_batch_var: missing array")
        msgs, msg_off, _, n = self._msg_items("schnorrsig_verify_batch_var", msgs, msg_off, None, None)
        sigs = _u8(sigs); pubkeys = _u8(pubkeys)
        _need("schnorrsig_verify_batch_var sigs", sigs, 64 * n); _need("schnorrsig_verify_batch_var pubkeys", pubkeys, (64 if pk_format else 32) * n)
        res = np.zeros(n, np.int32)
        pad = msgs if msgs.size else np.zeros(1, np.uint8)
        self._check(self._lib.secp256k1_schnorrsig_verify_batch_var(self._h, _p(res), _p(sigs), _p(pad), _p(msg_off), _p(pubkeys), pk_format, n),
                    "secp256k1_schnorrsig_verify_batch_var")
        return res

    def schnorrsig_verify_batch_var_dev(self, results, sigs, msgs, msg_off, pubkeys, pk_format=0, n=None, stream=None):
        """every array in HBM (torch tensors; msg_off: int64 / uint64 offsets[n+1]).  An item whose offsets decrease gets 0."""
        if pk_format not in (0, 1):
            raise ValueError("schnorrsig_verify_batch_var_dev: pk_format must be 0 or 1")
        if msg_off is None:
            raise ValueError("schnorrsig_verify_batch_var_dev: msg_off is required")
        _, n = self._msg_items_dev("schnorrsig_verify_batch_var_dev", msg_off, None, msgs, n)
        self._check(self._lib.secp256k1_schnorrsig_verify_batch_var_dev(self._h, stream, _dp(results), _dp(sigs), _dp(msgs), _dp(msg_off), _dp(pubkeys), pk_format, n),
                    "secp256k1_schnorrsig_verify_batch_var_dev")

    # ---- secp256k1_ellswift_decode and secp256k1_ellswift_encode (modules/ellswift/main_impl.h:470-483, :393-420), batched ----
    def ellswift_decode(self, ell64, out_format=1):
        """ell64: n*64 ElligatorSwift encodings -> out[n, 32 / 64 / 33]: out_format 0: ser32(x), 1: secp256k1_pubkey objects, 2: compressed keys.
        Every input decodes."""
        ell64, n = _ellswift_decode_args("ellswift_decode", ell64, out_format)
        out = np.zeros((n, _ELLSWIFT_OUT_BYTES[out_format]), np.uint8)
        self._check(self._lib.secp256k1_ellswift_decode_batch(self._h, _p(out), out_format, _p(ell64), n), "secp256k1_ellswift_decode_batch")
        return out

    def ellswift_decode_dev(self, out, ell64, out_format=1, n=None, stream=None):
        """every array in HBM (torch tensors)"""
        n = ell64.numel() // 64 if n is None else n
        self._check(self._lib.secp256k1_ellswift_decode_batch_dev(self._h, stream, _dp(out), out_format, _dp(ell64), n), "secp256k1_ellswift_decode_batch_dev")

    def ellswift_encode(self, keys, rnd32, key_format=1):
        """keys: key_format 1: n*64 secp256k1_pubkey objects, 2: n*33 compressed keys; rnd32: n*32 bytes of PUBLIC randomness
        -> (results[n], ell64[n, 64]), zero where results[i] == 0 (a refused key, or the attempt cap: ellswift_capped())"""
        keys, rnd32, n = _ellswift_encode_args("ellswift_encode", keys, key_format, rnd32)
        res = np.zeros(n, np.int32); out = np.zeros((n, 64), np.uint8)
        self._check(self._lib.secp256k1_ellswift_encode_batch(self._h, _p(res), _p(out), _p(keys), key_format, _p(rnd32), n), "secp256k1_ellswift_encode_batch")
        return res, out

    def ellswift_encode_dev(self, results, ell64_out, keys, rnd32, key_format=1, n=None, stream=None):
        """every array in HBM (torch tensors)"""
        n = rnd32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_ellswift_encode_batch_dev(self._h, stream, _dp(results), _dp(ell64_out), _dp(keys), key_format, _dp(rnd32), n),
                    "secp256k1_ellswift_encode_batch_dev")

    def ellswift_capped(self):
        """items of this engine's encode calls that hit the attempt cap so far (s2k_engine_ellswift_capped; waits for the device)"""
        c = ctypes.c_uint64(0)
        self._check(self._lib.s2k_engine_ellswift_capped(self._h, ctypes.byref(c)), "s2k_engine_ellswift_capped")
        return int(c.value)

    # ---- secp256k1_generator_generate[_blinded] / _parse / _serialize and secp256k1_pedersen_commit (modules/generator/main_impl.h:59-335), batched.
    #      Public inputs only: blinds are treated as public data (nothing is constant time). ----
    def generator_generate_batch(self, keys32, blinds32=None):
        """keys32: n*32 asset ids; blinds32: None or n*32 -> (results[n], gens64[n, 64]): secp256k1_generator objects, zero where results[i] == 0"""
        if keys32 is None:
            raise ValueError("generator_generate_batch: missing array")
        keys32 = _u8(keys32); n = keys32.size // 32
        _need("generator_generate_batch keys32", keys32, 32 * n)
        if blinds32 is not None:
            blinds32 = _u8(blinds32); _need("generator_generate_batch blinds32", blinds32, 32 * n)
        res = np.zeros(n, np.int32); gens = np.zeros((n, 64), np.uint8)
        self._check(self._lib.secp256k1_generator_generate_batch(self._h, _p(res), _p(gens), _p(keys32), _p(blinds32), n), "secp256k1_generator_generate_batch")
        return res, gens

    def generator_generate_batch_dev(self, results, gens_out64, keys32, blinds32=None, n=None, stream=None):
        """every array in HBM (torch tensors); blinds32 may be None"""
        n = keys32.numel() // 32 if n is None else n
        self._check(self._lib.secp256k1_generator_generate_batch_dev(self._h, stream, _dp(results), _dp(gens_out64), _dp(keys32), _dp(blinds32), n),
                    "secp256k1_generator_generate_batch_dev")

    def generator_parse_batch(self, gens33):
        """gens33: n*33 serialised generators (0x0a / 0x0b, x) -> (results[n], gens64[n, 64]), zero where refused"""
        if gens33 is None:
            raise ValueError("generator_parse_batch: missing array")
        gens33 = _u8(gens33); n = gens33.size // 33
        _need("generator_parse_batch gens33", gens33, 33 * n)
        res = np.zeros(n, np.int32); gens = np.zeros((n, 64), np.uint8)
        self._check(self._lib.secp256k1_generator_parse_batch(self._h, _p(res), _p(gens), _p(gens33), n), "secp256k1_generator_parse_batch")
        return res, gens

    def generator_parse_batch_dev(self, results, gens_out64, gens33, n=None, stream=None):
        n = gens33.numel() // 33 if n is None else n
        self._check(self._lib.secp256k1_generator_parse_batch_dev(self._h, stream, _dp(results), _dp(gens_out64), _dp(gens33), n), "secp256k1_generator_parse_batch_dev")

    def generator_serialize_batch(self, gens64):
        """gens64: n*64 secp256k1_generator objects -> out33[n, 33]"""
        if gens64 is None:
            raise ValueError("generator_serialize_batch: missing array")
        gens64 = _u8(gens64); n = gens64.size // 64
        _need("generator_serialize_batch gens64", gens64, 64 * n)
        out = np.zeros((n, 33), np.uint8)
        self._check(self._lib.secp256k1_generator_serialize_batch(self._h, _p(out), _p(gens64), n), "secp256k1_generator_serialize_batch")
        return out

    def generator_serialize_batch_dev(self, out33, gens64, n=None, stream=None):
        n = gens64.numel() // 64 if n is None else n
        self._check(self._lib.secp256k1_generator_serialize_batch_dev(self._h, stream, _dp(out33), _dp(gens64), n), "secp256k1_generator_serialize_batch_dev")

    def pedersen_commit_batch(self, values, gens64, blinds32=None):
        """values: n uint64; gens64: n*64 generator objects; blinds32: None (all-zero blinds: explicit amounts) or n*32
        -> (results[n], commits33[n, 33]): serialised commitments, zero where results[i] == 0"""
        if values is None or gens64 is None:
            raise ValueError("pedersen_commit_batch: missing array")
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1); n = values.size
        gens64 = _u8(gens64); _need("pedersen_commit_batch gens64", gens64, 64 * n)
        if blinds32 is not None:
            blinds32 = _u8(blinds32); _need("pedersen_commit_batch blinds32", blinds32, 32 * n)
        res = np.zeros(n, np.int32); out = np.zeros((n, 33), np.uint8)
        self._check(self._lib.secp256k1_pedersen_commit_batch(self._h, _p(res), _p(out), _p(blinds32), _p(values), _p(gens64), n), "secp256k1_pedersen_commit_batch")
        return res, out

    def pedersen_commit_batch_dev(self, results, commits_out33, values, gens64, blinds32=None, n=None, stream=None):
        """every array in HBM (torch tensors; values int64 or uint64 bit patterns); blinds32 may be None"""
        n = values.numel() if n is None else n
        self._check(self._lib.secp256k1_pedersen_commit_batch_dev(self._h, stream, _dp(results), _dp(commits_out33), _dp(blinds32), _dp(values), _dp(gens64), n),
                    "secp256k1_pedersen_commit_batch_dev")

    # ---- secp256k1_whitelist_signature_parse + secp256k1_whitelist_verify (modules/whitelist/main_impl.h:99-151), batched ----
    @staticmethod
    def _whitelist_lists(what, lists_online, lists_offline, list_off, list_of, n):
        """the key lists as the C call wants them: (online, offline, list_off[n_lists+1], n_lists, list_of or None)"""
        if list_off is None:                                          # a list of per-list byte strings
            online, list_off = Engine.pack([bytes(_u8(x)) for x in lists_online])
            offline, off2 = Engine.pack([bytes(_u8(x)) for x in lists_offline])
            if not np.array_equal(list_off, off2) or (list_off % 64).any():
                raise ValueError(f"{what}: online and offline lists must have the same lengths, 64 bytes per key")
            list_off = list_off // np.uint64(64)
        else:                                                         # already packed: keys back to back, list_off in keys
            online, offline = _u8(lists_online), _u8(lists_offline)
            list_off = np.ascontiguousarray(list_off, dtype=np.uint64)
            if list_off.size == 0:
                raise ValueError(f"{what}: list_off needs n_lists + 1 entries")
        n_lists = list_off.size - 1
        keys = int(list_off.max())
        if online.size < 64 * keys or offline.size < 64 * keys:
            raise ValueError(f"{what}: the key arrays are shorter than list_off says")
        if list_of is None:
            if n_lists != n:
                raise ValueError(f"{what}: without list_of there must be one list per item")
        else:
            list_of = np.ascontiguousarray(list_of, dtype=np.uint32)
            _need(what + " list_of", list_of, n)
        return online, offline, list_off, n_lists, list_of

    def whitelist_verify_batch(self, sigs, lists_online, lists_offline, subs64, list_of=None, list_off=None):
        """sigs: a list of serialised signatures (packed here) or the tuple (data, offsets[n+1]); lists_online / lists_offline: a list of
        per-list byte strings of 64-byte secp256k1_pubkey objects, or -- with list_off[n_lists+1], counted in keys -- the packed arrays;
        list_of[n]: each item's list (None: list i for item i); subs64: n*64.  What the C call refuses (a list_of entry out of range,
        decreasing list_off) is refused there: S2KError."""
        what = "whitelist_verify_batch"
        if isinstance(sigs, tuple) and len(sigs) == 2:
            data, off = _u8(sigs[0]), np.ascontiguousarray(sigs[1], dtype=np.uint64)
        else:
            data, off = Engine.pack([bytes(x) for x in sigs])
        n = off.size - 1
        _offsets_ok(what + " sigs", off, data.size)
        subs64 = _u8(subs64); _need(what + " subs64", subs64, 64 * n)
        online, offline, list_off, n_lists, list_of = self._whitelist_lists(what, lists_online, lists_offline, list_off, list_of, n)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_whitelist_verify_batch(self._h, _p(res), _p(data), _p(off), _p(online), _p(offline), _p(list_off), n_lists, _p(list_of),
                                                               _p(subs64), n), "secp256k1_whitelist_verify_batch")
        return res

    def whitelist_verify_batch_dev(self, results, sigs, sig_off, online64, offline64, list_off, subs64, list_of=None, stream=None):
        """results, sigs, online64, offline64, subs64 in HBM (torch tensors); sig_off[n+1], list_off[n_lists+1] and list_of[n] are HOST
        arrays (numpy), read before the call returns"""
        sig_off = np.ascontiguousarray(sig_off, dtype=np.uint64); list_off = np.ascontiguousarray(list_off, dtype=np.uint64)
        n = sig_off.size - 1
        if list_of is not None:
            list_of = np.ascontiguousarray(list_of, dtype=np.uint32)
            _need("whitelist_verify_batch_dev list_of", list_of, n)
        self._check(self._lib.secp256k1_whitelist_verify_batch_dev(self._h, stream, _dp(results), _dp(sigs), _p(sig_off), _dp(online64), _dp(offline64), _p(list_off),
                                                                   list_off.size - 1, _p(list_of), _dp(subs64), n), "secp256k1_whitelist_verify_batch_dev")

    def bppp_norm_product_verify_batch_dev(self, results, proofs, proof_len, transcripts, rho, gens33_dev, gens33_host, g_len, c_vec, c_vec_len, commits33, n,
                                           stream=None):
        """every array in HBM (torch uint8 tensors); gens33_host: the same generator set as a numpy array (cache key of the fixed-base table)"""
        gh = _u8(gens33_host)
        self._check(self._lib.secp256k1_bppp_norm_product_verify_batch_dev(self._h, stream, _dp(results), _dp(proofs), proof_len, _dp(transcripts), _dp(rho), _dp(gens33_dev),
                                                                            _p(gh), gh.size // 33, g_len, _dp(c_vec), c_vec_len, _dp(commits33), n),
                    "secp256k1_bppp_norm_product_verify_batch_dev")

    # ---- secp256k1_bppp_commit (modules/bppp/bppp_norm_product_impl.h:105-151), batched on the fixed-base tables -----
    def bppp_commit_batch(self, gens33, g_len, n_vec, l_vec, c_vec, mu):
        """gens33 (n_gens,33); n_vec (n,g_len,32); l_vec, c_vec (n,h_len,32); mu (n,32) -> (commits (n,33), set_ok (n,))"""
        gens33 = _u8(gens33); n_gens = gens33.size // 33
        mu = _u8(mu); n = mu.size // 32
        h_len = n_gens - g_len
        n_vec = _u8(n_vec); l_vec = _u8(l_vec); c_vec = _u8(c_vec)
        if n_vec.size != n * g_len * 32 or l_vec.size != n * h_len * 32 or c_vec.size != n * h_len * 32:
            raise ValueError("bppp_commit_batch: vector shapes do not match (n, g_len, h_len)")
        out = np.zeros((n, 33), np.uint8); res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_bppp_commit_batch(self._h, _p(out), _p(res), _p(gens33), n_gens, g_len, _p(n_vec), _p(l_vec), _p(c_vec), h_len, _p(mu), n),
                    "secp256k1_bppp_commit_batch")
        return out, res

    # ---- secp256k1_schnorrsig_aggverify (modules/schnorrsig_halfagg/main_impl.h:108-198) as one MSM -------------
    def schnorrsig_aggverify(self, pubkeys, msgs32, aggsig, pk_format=0, n=None):
        """pubkeys: (n,32) serialised x-only keys (or (n,64) objects with pk_format=1); msgs32: (n,32); aggsig: bytes r_0..r_{n-1}|s.
        n defaults to the number of messages.  Returns the reference's verdict (0/1)."""
        pubkeys = _u8(pubkeys); msgs32 = _u8(msgs32); aggsig = _u8(aggsig)
        if n is None:
            n = msgs32.size // 32
        if msgs32.size < 32 * n or pubkeys.size < (64 if pk_format else 32) * n:
            raise ValueError("schnorrsig_aggverify: fewer keys / messages than n")
        res = np.zeros(1, np.int32)
        self._check(self._lib.secp256k1_schnorrsig_aggverify_amd(self._h, _p(res), _p(pubkeys) if n else None, pk_format, _p(msgs32) if n else None, n,
                                                                 _p(aggsig), aggsig.size), "secp256k1_schnorrsig_aggverify_amd")
        return int(res[0])

    # ---- many half-aggregates per call (include/secp256k1_zkp_amd.h: verification as K sums in one launch chain, and aggregation) ----
    @staticmethod
    def _halfagg_items(what, keys, msgs, pk_format):
        """lists of per-aggregate byte strings -> (keys array, msgs array, item_off, counts)"""
        if pk_format not in (0, 1):
            raise ValueError(f"{what}: pk_format must be 0 (32-byte x-only keys) or 1 (64-byte objects)")
        if keys is None or msgs is None or len(keys) != len(msgs):
            raise ValueError(f"{what}: one key string and one message string per aggregate")
        pkb = 64 if pk_format else 32
        counts = []
        for k, (pk, m) in enumerate(zip(keys, msgs)):
            pk, m = bytes(pk), bytes(m)
            if len(m) % 32 or len(pk) != pkb * (len(m) // 32):
                raise ValueError(f"{what}: aggregate {k} needs 32 message bytes and {pkb} key bytes per signature")
            counts.append(len(m) // 32)
        off = np.zeros(len(counts) + 1, np.uint64); off[1:] = np.cumsum(np.array(counts, np.uint64), dtype=np.uint64)
        return _u8(b"".join(bytes(x) for x in keys)), _u8(b"".join(bytes(x) for x in msgs)), off, counts

    def schnorrsig_aggverify_batch(self, pubkeys, msgs32, aggsigs, pk_format=0):
        """pubkeys, msgs32, aggsigs: lists with one byte string per aggregate (n_k keys, n_k messages, r_0..r_{n_k-1}|s).  Returns int32
        verdicts, the reference's secp256k1_schnorrsig_aggverify per aggregate (a wrong-length aggregate gets 0)."""
        keys, msgs, off, counts = self._halfagg_items("schnorrsig_aggverify_batch", pubkeys, msgs32, pk_format)
        if aggsigs is None or len(aggsigs) != len(counts):
            raise ValueError("schnorrsig_aggverify_batch: one aggregate per key string")
        agg, agg_off = self.pack([bytes(a) for a in aggsigs])
        n = len(counts); res = np.zeros(max(n, 1), np.int32)
        self._check(self._lib.secp256k1_schnorrsig_aggverify_batch(self._h, _p(res), _p(keys) if keys.size else None, pk_format, _p(msgs) if msgs.size else None, _p(off),
                                                                   _p(agg) if agg.size else _p(np.zeros(1, np.uint8)), _p(agg_off), n), "secp256k1_schnorrsig_aggverify_batch")
        return res[:n]

    def schnorrsig_inc_aggregate_batch(self, aggsigs_in, pubkeys, msgs32, new_sigs64, pk_format=0):
        """aggsigs_in: per aggregate the 32 (n_before + 1) bytes it already has (None: the plain aggregation, n_before = 0 everywhere);
        pubkeys, msgs32: ALL n_k keys and messages per aggregate; new_sigs64: the n_k - n_before new signatures per aggregate.
        Returns (verdicts, list of aggregates: 32 (n_k + 1) bytes each, all zero where the verdict is 0)."""
        what = "schnorrsig_inc_aggregate_batch"
        keys, msgs, off, counts = self._halfagg_items(what, pubkeys, msgs32, pk_format)
        n = len(counts)
        if new_sigs64 is None or len(new_sigs64) != n or (aggsigs_in is not None and len(aggsigs_in) != n):
            raise ValueError(f"{what}: one string per aggregate in every list")
        before = []
        for k in range(n):
            old = 0
            if aggsigs_in is not None:
                ln = len(bytes(aggsigs_in[k]))
                if ln % 32 or ln == 0:
                    raise ValueError(f"{what}: aggregate {k} of aggsigs_in must be 32 (n_before + 1) bytes")
                old = ln // 32 - 1
            ns = len(bytes(new_sigs64[k]))
            if ns % 64 or old + ns // 64 != counts[k]:
                raise ValueError(f"{what}: aggregate {k} has {counts[k]} keys but {old} + {ns // 64} signatures")
            before.append(old)
        sigs = _u8(b"".join(bytes(x) for x in new_sigs64))
        res = np.zeros(max(n, 1), np.int32); out = np.zeros(32 * (int(off[-1]) + n) + 1, np.uint8)
        if aggsigs_in is None:
            ok = self._lib.secp256k1_schnorrsig_aggregate_batch(self._h, _p(res), _p(out), _p(keys) if keys.size else None, pk_format, _p(msgs) if msgs.size else None,
                                                                _p(sigs) if sigs.size else None, _p(off), n)
            self._check(ok, "secp256k1_schnorrsig_aggregate_batch")
        else:
            old = _u8(b"".join(bytes(x) for x in aggsigs_in)); nb = np.array(before + [0], np.uint64)
            ok = self._lib.secp256k1_schnorrsig_inc_aggregate_batch(self._h, _p(res), _p(out), _p(old) if old.size else _p(np.zeros(1, np.uint8)), _p(nb),
                                                                    _p(keys) if keys.size else None, pk_format, _p(msgs) if msgs.size else None,
                                                                    _p(sigs) if sigs.size else None, _p(off), n)
            self._check(ok, "secp256k1_schnorrsig_inc_aggregate_batch")
        return res[:n], [out[32 * (int(off[k]) + k):32 * (int(off[k + 1]) + k + 1)].tobytes() for k in range(n)]

    def schnorrsig_aggregate_batch(self, pubkeys, msgs32, sigs64, pk_format=0):
        """lists with one byte string per aggregate (n_k keys, messages, 64-byte signatures) -> (verdicts, list of 32 (n_k + 1)-byte aggregates)"""
        return self.schnorrsig_inc_aggregate_batch(None, pubkeys, msgs32, sigs64, pk_format)

    # ---- secp256k1_pedersen_verify_tally (modules/generator/main_impl.h:371-396), batched -------------------------
    def pedersen_verify_tally_batch(self, tallies):
        """tallies: list of (positive, negative), each a (k,33) uint8 array (or list of 33-byte strings) of serialised commitments.
        Returns int32[n]."""
        parts, off, npos = [], [0], []
        for pos, neg in tallies:
            pos = _u8(b"".join(bytes(x) for x in pos) if isinstance(pos, (list, tuple)) else pos).reshape(-1, 33)
            neg = _u8(b"".join(bytes(x) for x in neg) if isinstance(neg, (list, tuple)) else neg).reshape(-1, 33)
            parts += [pos, neg]; npos.append(pos.shape[0]); off.append(off[-1] + pos.shape[0] + neg.shape[0])
        n = len(tallies)
        data = np.ascontiguousarray(np.concatenate(parts)) if parts and off[-1] else np.zeros((1, 33), np.uint8)
        off = np.array(off, np.uint64); npos = np.array(npos + [0], np.uint64)
        res = np.zeros(max(n, 1), np.int32)
        self._check(self._lib.secp256k1_pedersen_verify_tally_batch(self._h, _p(res), _p(data), _p(off), _p(npos), n), "secp256k1_pedersen_verify_tally_batch")
        return res[:n]

    # ---- secp256k1_rangeproof_verify (modules/rangeproof/main_impl.h:54-71), batched ---------------------------
    @staticmethod
    def pack(items):
        """list of bytes -> (concatenated uint8 array, uint64 offsets[n+1])"""
        off = np.zeros(len(items) + 1, np.uint64)
        if items:
            off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8).copy()
        return data, off

    def rangeproof_verify_batch(self, commits33, proofs, gens64, extra=None):
        """commits33: (n,33) uint8; proofs: list of bytes or (data, offsets); gens64: (n,64); extra: optional list of bytes.
        Returns (results int32[n], min_value uint64[n], max_value uint64[n])."""
        data, off = proofs if isinstance(proofs, tuple) else self.pack(list(proofs))
        n = off.size - 1
        commits33 = _u8(commits33); gens64 = _u8(gens64)
        edata = eoff = None
        if extra is not None:
            edata, eoff = extra if isinstance(extra, tuple) else self.pack(list(extra))
        self._check_rp_shapes("rangeproof_verify_batch", n, commits33, gens64, data, off, edata, eoff)
        res = np.zeros(n, np.int32); mn = np.zeros(n, np.uint64); mx = np.zeros(n, np.uint64)
        self._check(self._lib.secp256k1_rangeproof_verify_batch(self._h, _p(res), _p(mn), _p(mx), _p(commits33), _p(data), _p(off),
                                                                 _p(edata), _p(eoff), _p(gens64), n), "secp256k1_rangeproof_verify_batch")
        return res, mn, mx

    def rangeproof_verify_batch_submit(self, commits33, proofs, gens64, extra=None):
        """Asynchronous form: gathers and queues the batch, returns a ticket object; `rangeproof_verify_batch_wait(ticket)` returns
        (results, min_value, max_value).  At most two tickets may be outstanding (include/secp256k1_zkp_amd.h)."""
        data, off = proofs if isinstance(proofs, tuple) else self.pack(list(proofs))
        n = off.size - 1
        commits33 = _u8(commits33); gens64 = _u8(gens64)
        edata = eoff = None
        if extra is not None:
            edata, eoff = extra if isinstance(extra, tuple) else self.pack(list(extra))
        self._check_rp_shapes("rangeproof_verify_batch_submit", n, commits33, gens64, data, off, edata, eoff)
        res = np.zeros(n, np.int32); mn = np.zeros(n, np.uint64); mx = np.zeros(n, np.uint64)
        t = ctypes.c_uint64(0)
        self._check(self._lib.secp256k1_rangeproof_verify_batch_submit(self._h, ctypes.byref(t), _p(res), _p(mn), _p(mx), _p(commits33), _p(data), _p(off),
                                                                        _p(edata), _p(eoff), _p(gens64), n), "secp256k1_rangeproof_verify_batch_submit")
        return (t.value, res, mn, mx)                  # the output arrays live in the ticket until it is waited for

    def rangeproof_verify_batch_wait(self, ticket):
        t, res, mn, mx = ticket
        self._check(self._lib.secp256k1_rangeproof_verify_batch_wait(self._h, ctypes.c_uint64(t)), "secp256k1_rangeproof_verify_batch_wait")
        return res, mn, mx

    @staticmethod
    def _check_rp_shapes(what, n, commits33, gens64, data, off, edata, eoff):
        _need(what + " commits33", commits33, 33 * n); _need(what + " gens64", gens64, 64 * n)
        if np.asarray(off).size != n + 1:
            raise ValueError(what + ": proof offsets must have n + 1 entries")
        _offsets_ok(what + " proofs", off, data.size)
        if eoff is not None:
            if np.asarray(eoff).size != n + 1:
                raise ValueError(what + ": extra_commit offsets must have n + 1 entries")
            _offsets_ok(what + " extra", eoff, edata.size)

    def rangeproof_rewind_batch(self, commits33, proofs, gens64, nonces, msg_capacity=4096, extra=None):
        """secp256k1_rangeproof_rewind per item.  Returns (results, blinds (n,32), values uint64[n], messages list[bytes], min, max)."""
        data, off = proofs if isinstance(proofs, tuple) else self.pack(list(proofs))
        n = off.size - 1
        commits33 = _u8(commits33); gens64 = _u8(gens64); nonces = _u8(nonces)
        edata = eoff = None
        if extra is not None:
            edata, eoff = extra if isinstance(extra, tuple) else self.pack(list(extra))
        self._check_rp_shapes("rangeproof_rewind_batch", n, commits33, gens64, data, off, edata, eoff)
        _need("rangeproof_rewind_batch nonces", nonces, 32 * n)
        res = np.zeros(n, np.int32); mn = np.zeros(n, np.uint64); mx = np.zeros(n, np.uint64)
        blind = np.zeros((n, 32), np.uint8); val = np.zeros(n, np.uint64)
        msg = np.zeros((n, max(msg_capacity, 1)), np.uint8) if msg_capacity else None
        ol = np.full(n, msg_capacity, np.uint64)
        self._check(self._lib.secp256k1_rangeproof_rewind_batch(self._h, _p(res), _p(blind), _p(val), _p(msg), _p(ol) if msg_capacity else None, msg_capacity,
                                                                 _p(nonces), _p(mn), _p(mx), _p(commits33), _p(data), _p(off), _p(edata), _p(eoff), _p(gens64), n),
                    "secp256k1_rangeproof_rewind_batch")
        msgs = [msg[i, :int(ol[i])].tobytes() if (msg_capacity and res[i]) else b"" for i in range(n)]
        return res, blind, val, msgs, mn, mx

    def rangeproof_verify_batch_dev(self, results, min_value, max_value, commits33, proofs, proof_off, gens64, n, extra=None, extra_off=None,
                                    stream=None):
        self._check(self._lib.secp256k1_rangeproof_verify_batch_dev(self._h, stream, _dp(results), _dp(min_value), _dp(max_value), _dp(commits33),
                                                                     _dp(proofs), _dp(proof_off), _dp(extra), _dp(extra_off), _dp(gens64), n),
                    "secp256k1_rangeproof_verify_batch_dev")

    # ---- secp256k1_surjectionproof_verify (modules/surjection/main_impl.h:360-402), batched ---------------------
    def surjectionproof_verify_batch(self, proofs, input_tags, output_tags64):
        """proofs: list of serialised proofs; input_tags: list of (k_i,64) uint8 arrays; output_tags64: (n,64)."""
        data, off = self.pack(list(proofs))
        n = off.size - 1
        toff = np.zeros(n + 1, np.uint64)
        toff[1:] = np.cumsum([np.asarray(t).size // 64 for t in input_tags], dtype=np.uint64)
        tags = np.concatenate([_u8(t).reshape(-1) for t in input_tags] + [np.zeros(64, np.uint8)])
        if len(input_tags) != n:
            raise ValueError("surjectionproof_verify_batch: one input-tag list per proof")
        _need("surjectionproof_verify_batch output_tags64", _u8(output_tags64), 64 * n)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_surjectionproof_verify_batch(self._h, _p(res), _p(data), _p(off), _p(tags), _p(toff), _p(_u8(output_tags64)), n),
                    "secp256k1_surjectionproof_verify_batch")
        return res

    # ---- secp256k1_bppp_rangeproof_norm_product_verify (modules/bppp/bppp_norm_product_impl.h:425-552), batched --
    def bppp_norm_product_verify_batch(self, proofs, transcripts, rho, gens33, g_len, c_vec, commits33):
        proofs = _u8(proofs); n = _u8(rho).size // 32
        proof_len = proofs.size // max(n, 1)
        gens33 = _u8(gens33); n_gens = gens33.size // 33
        c_vec = _u8(c_vec); c_len = c_vec.size // 32 // max(n, 1)
        _need("bppp_norm_product_verify_batch proofs", proofs, proof_len * n); _need("bppp_norm_product_verify_batch transcripts", _u8(transcripts), 104 * n)
        _need("bppp_norm_product_verify_batch c_vec", c_vec, 32 * c_len * n); _need("bppp_norm_product_verify_batch commits33", _u8(commits33), 33 * n)
        _need("bppp_norm_product_verify_batch gens33", gens33, 33 * n_gens)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_bppp_norm_product_verify_batch(self._h, _p(res), _p(proofs), proof_len, _p(_u8(transcripts)), _p(_u8(rho)),
                                                                        _p(gens33), n_gens, g_len, _p(c_vec), c_len, _p(_u8(commits33)), n),
                    "secp256k1_bppp_norm_product_verify_batch")
        return res

    # ---- one verdict for a whole batch of norm arguments over one generator set, as a single multi-scalar multiplication (csrc/bppp_all.h) ----
    def bppp_norm_product_verify_all(self, proofs, transcripts, rho, gens33, g_len, c_vec, commits33, locate=False, want_seed=False):
        """1 exactly when every proof of the batch verifies (arguments as bppp_norm_product_verify_batch).  Returns the verdict; with locate=True
        (verdict, results) where results are the per-proof verdicts (all ones when the verdict is 1); with want_seed=True the 32-byte seed of
        the coefficients is appended."""
        what = "bppp_norm_product_verify_all"
        if proofs is None or transcripts is None or rho is None or gens33 is None or c_vec is None or commits33 is None:
            raise ValueError(what + ": missing array")
        if g_len < 0:
            raise ValueError(what + ": g_len must not be negative")
        proofs = _u8(proofs); transcripts = _u8(transcripts); rho = _u8(rho); gens33 = _u8(gens33); c_vec = _u8(c_vec); commits33 = _u8(commits33)
        n = rho.size // 32; n_gens = gens33.size // 33
        proof_len = proofs.size // max(n, 1); c_len = c_vec.size // 32 // max(n, 1)
        _need(what + " rho", rho, 32 * n); _need(what + " proofs", proofs, proof_len * n); _need(what + " transcripts", transcripts, 104 * n)
        _need(what + " c_vec", c_vec, 32 * c_len * n); _need(what + " commits33", commits33, 33 * n); _need(what + " gens33", gens33, 33 * n_gens)
        if n and (proof_len == 0 or c_len == 0 or n_gens == 0):
            raise ValueError(what + ": empty proofs, c_vec or generator set")
        verdict = np.zeros(1, np.int32); res = np.zeros(max(n, 1), np.int32) if locate else None; seed = np.zeros(32, np.uint8) if want_seed else None
        nz = lambda a: _p(a) if n else None
        self._check(self._lib.secp256k1_bppp_norm_product_verify_all(self._h, _p(verdict), _p(res), _p(seed), nz(proofs), proof_len, nz(transcripts), nz(rho), nz(gens33),
                                                                     n_gens, g_len, nz(c_vec), c_len, nz(commits33), n), "secp256k1_" + what)
        out = (int(verdict[0]),) + ((res[:n],) if locate else ()) + ((seed.tobytes(),) if want_seed else ())
        return out[0] if len(out) == 1 else out

    def bppp_norm_product_verify_all_dev(self, verdict, proofs, proof_len, transcripts, rho, gens33_dev, gens33_host, g_len, c_vec, c_vec_len, commits33, n,
                                         seed_out=None, stream=None):
        """every array in HBM (torch tensors): verdict int32[1], seed_out uint8[32] or None; gens33_host: the same generator set as a numpy array
        (it is hashed on the host); nothing is read back"""
        what = "bppp_norm_product_verify_all_dev"
        if verdict is None or verdict.numel() < 1 or (seed_out is not None and seed_out.numel() < 32):
            raise ValueError(what + ": verdict needs one int32 and seed_out 32 bytes")
        if n < 0 or proof_len < 0 or c_vec_len < 0 or g_len < 0:
            raise ValueError(what + ": negative size")
        gh = _u8(gens33_host) if gens33_host is not None else None
        if n:
            if gh is None or gh.size % 33 or gens33_dev is None or gens33_dev.numel() < gh.size:
                raise ValueError(what + ": the generator set is needed on the host and on the device, 33 bytes per generator")
            if (proofs is None or transcripts is None or rho is None or c_vec is None or commits33 is None or proofs.numel() < proof_len * n or transcripts.numel() < 104 * n
                    or rho.numel() < 32 * n or c_vec.numel() < 32 * c_vec_len * n or commits33.numel() < 33 * n):
                raise ValueError(what + ": fewer proof / transcript / rho / c_vec / commitment bytes than n needs")
        nz = lambda t: _dp(t) if n else None
        self._check(self._lib.secp256k1_bppp_norm_product_verify_all_dev(self._h, stream, _dp(verdict), _dp(seed_out), nz(proofs), proof_len, nz(transcripts), nz(rho),
                                                                         nz(gens33_dev), _p(gh) if n else None, gh.size // 33 if gh is not None else 0, g_len, nz(c_vec),
                                                                         c_vec_len, nz(commits33), n), "secp256k1_" + what)

    def bppp_all_last_split_ms(self):
        """[per-proof scalars + item digests, tree + seed + z', column sums + own terms, MSM] of the most recent verify_all call, in ms (after sync())"""
        out = np.full(4, -1.0, np.float32)
        self._check(self._lib.s2k_bppp_all_last_split_ms(self._h, _p(out)), "s2k_bppp_all_last_split_ms")
        return [float(x) for x in out]


class Group:
    """The GPUs of one node behind one handle (s2k_group, include/secp256k1_zkp_amd.h): one engine and one host thread per entry of
    `devices`; batches of independent items are cut into contiguous ranges, one large multi-scalar multiplication is sharded by terms."""

    def __init__(self, devices):
        self._lib = _native.load()
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._h = self._lib.s2k_group_create(devs, len(devices))
        if not self._h:
            raise S2KError("s2k_group_create failed: " + _native.last_error())
        self.devices = [int(d) for d in devices]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.s2k_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._lib.s2k_group_size(self._h))

    def _check(self, ok, what):
        if not ok:
            raise S2KError(f"{what} failed: {_native.last_error()}")

    def engine(self, i):
        """a non-owning Engine view of member i (options, generator cache)"""
        h = self._lib.s2k_group_engine(self._h, int(i))
        if not h:
            raise IndexError(i)
        e = Engine.__new__(Engine)
        e._lib = self._lib; e._h = h; e.device = self.devices[i]
        e.close = lambda: None                   # the group owns it
        return e

    def rangeproof_verify_batch(self, commits33, proofs, gens64, extra=None):
        data, off = proofs if isinstance(proofs, tuple) else Engine.pack(list(proofs))
        n = off.size - 1
        commits33 = _u8(commits33); gens64 = _u8(gens64)
        edata = eoff = None
        if extra is not None:
            edata, eoff = extra if isinstance(extra, tuple) else Engine.pack(list(extra))
        Engine._check_rp_shapes("rangeproof_verify_batch_group", n, commits33, gens64, data, off, edata, eoff)
        res = np.zeros(n, np.int32); mn = np.zeros(n, np.uint64); mx = np.zeros(n, np.uint64)
        self._check(self._lib.secp256k1_rangeproof_verify_batch_group(self._h, _p(res), _p(mn), _p(mx), _p(commits33), _p(data), _p(off), _p(edata), _p(eoff),
                                                                       _p(gens64), n), "secp256k1_rangeproof_verify_batch_group")
        return res, mn, mx

    def schnorrsig_verify_batch(self, sigs, msgs, pubkeys, msglen=32, pk_format=0):
        sigs = _u8(sigs); msgs = _u8(msgs); pubkeys = _u8(pubkeys); n = sigs.size // 64
        _need("schnorrsig_verify_batch_group sigs", sigs, 64 * n); _need("schnorrsig_verify_batch_group msgs", msgs, msglen * n)
        _need("schnorrsig_verify_batch_group pubkeys", pubkeys, (64 if pk_format else 32) * n)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_schnorrsig_verify_batch_group(self._h, _p(res), _p(sigs), _p(msgs), msglen, _p(pubkeys), pk_format, n),
                    "secp256k1_schnorrsig_verify_batch_group")
        return res

    def ecdsa_verify_batch(self, sigs, msghashes, pubkeys, sig_format=0, pk_format=0):
        sigs, off, msghashes, pubkeys, n = _ecdsa_args("ecdsa_verify_batch_group", sigs, msghashes, pubkeys, sig_format, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_verify_batch_group(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(msghashes), _p(pubkeys), pk_format, n),
                    "secp256k1_ecdsa_verify_batch_group")
        return res

    def musig_partial_sig_verify(self, partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of=None, sig_format=0, nonce_format=0, pk_format=0):
        partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, ns, n = _musig_verify_args(
            "musig_partial_sig_verify_group", partial_sigs, pubnonces, pubkeys, keyagg_caches, sessions, session_of, sig_format, nonce_format, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_musig_partial_sig_verify_batch_group(self._h, _p(res), _p(partial_sigs), sig_format, _p(pubnonces), nonce_format, _p(pubkeys),
                                                                             pk_format, _p(keyagg_caches), _p(sessions), ns, _p(session_of), n),
                    "secp256k1_musig_partial_sig_verify_batch_group")
        return res

    def ecdsa_adaptor_verify_batch(self, adaptor_sigs, pubkeys, msgs32, enckeys, pk_format=0):
        adaptor_sigs, pubkeys, msgs32, enckeys, n = _adaptor_args("ecdsa_adaptor_verify_batch_group", adaptor_sigs, pubkeys, msgs32, enckeys, pk_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_adaptor_verify_batch_group(self._h, _p(res), _p(adaptor_sigs), _p(pubkeys), _p(msgs32), _p(enckeys), pk_format, n),
                    "secp256k1_ecdsa_adaptor_verify_batch_group")
        return res

    def ecdsa_s2c_verify_commit_batch(self, sigs, data32, openings, sig_format=0, opening_format=0):
        sigs, off, _, _, data32, openings, n = _s2c_args("ecdsa_s2c_verify_commit_batch_group", sigs, data32, openings, sig_format, opening_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_ecdsa_s2c_verify_commit_batch_group(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(data32), _p(openings), opening_format, n),
                    "secp256k1_ecdsa_s2c_verify_commit_batch_group")
        return res

    def anti_exfil_host_verify_batch(self, sigs, msghashes, pubkeys, host_data32, openings, sig_format=0, pk_format=0, opening_format=0):
        sigs, off, msghashes, pubkeys, host_data32, openings, n = _s2c_args("anti_exfil_host_verify_batch_group", sigs, host_data32, openings, sig_format, opening_format,
                                                                            msghashes, pubkeys, pk_format, full=True)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_anti_exfil_host_verify_batch_group(self._h, _p(res), _p(sigs), _p(off), sig_format, _p(msghashes), _p(pubkeys), pk_format,
                                                                           _p(host_data32), _p(openings), opening_format, n), "secp256k1_anti_exfil_host_verify_batch_group")
        return res

    def ellswift_decode(self, ell64, out_format=1):
        ell64, n = _ellswift_decode_args("ellswift_decode_group", ell64, out_format)
        out = np.zeros((n, _ELLSWIFT_OUT_BYTES[out_format]), np.uint8)
        self._check(self._lib.secp256k1_ellswift_decode_batch_group(self._h, _p(out), out_format, _p(ell64), n), "secp256k1_ellswift_decode_batch_group")
        return out

    def xonly_tweak_add_check_batch(self, tweaked32, parities, internal_keys, tweaks32, key_format=0):
        tweaked32, parities, internal_keys, tweaks32, n = _tweak_check_args("xonly_tweak_add_check_batch_group", tweaked32, parities, internal_keys, tweaks32, key_format)
        res = np.zeros(n, np.int32)
        self._check(self._lib.secp256k1_xonly_pubkey_tweak_add_check_batch_group(self._h, _p(res), _p(tweaked32), _p(parities), _p(internal_keys), key_format,
                                                                                  _p(tweaks32), n), "secp256k1_xonly_pubkey_tweak_add_check_batch_group")
        return res

    def pubkey_tweak_mul(self, keys, tweaks32, key_format=1, out_format=1):
        """Engine.pubkey_tweak_mul with the items shared out over the group's engines"""
        keys, tweaks32, n = _pk_tweak_mul_args("Group.pubkey_tweak_mul", keys, key_format, tweaks32, out_format)
        res = np.zeros(n, np.int32); out = np.zeros((n, _PK_BYTES[out_format]), np.uint8); par = np.zeros(n, np.uint8)
        self._check(self._lib.secp256k1_ec_pubkey_tweak_mul_batch_group(self._h, _p(res), _p(out), out_format, _p(par), _p(keys), key_format, _p(tweaks32), n),
                    "secp256k1_ec_pubkey_tweak_mul_batch_group")
        return res, out, par

    def ecmult_multi(self, sc, pt_xy, g_sc=None, pt_inf=None):
        sc = _u8(sc); pt_xy = _u8(pt_xy); n = sc.size // 32
        g_sc = None if g_sc is None else _u8(g_sc); pt_inf = None if pt_inf is None else _u8(pt_inf)
        _need("ecmult_multi_group sc", sc, 32 * n); _need("ecmult_multi_group pt_xy", pt_xy, 64 * n)
        if g_sc is not None: _need("ecmult_multi_group g_sc", g_sc, 32)
        if pt_inf is not None: _need("ecmult_multi_group pt_inf", pt_inf, n)
        r = np.zeros(64, np.uint8); inf = np.zeros(1, np.int32)
        self._check(self._lib.s2k_ecmult_multi_group(self._h, _p(r), _p(inf), _p(g_sc), _p(sc), _p(pt_xy), _p(pt_inf), n), "s2k_ecmult_multi_group")
        return r, int(inf[0])

    def ecmult_multi_many(self, sc, pt_xy, offsets, g_sc=None, pt_inf=None):
        """K independent sums over the members of the group (s2k_ecmult_multi_many per member): the sums are independent objects, so they are
        cut into contiguous ranges of about equal numbers of TERMS, one range per member, one host thread per member (the call releases
        the GIL) -- no exchange between the GPUs, results in the caller's order.  A C caller does the same split over the engines of its
        s2k_group (s2k_group_engine); the reference has no counterpart (one sum per secp256k1_ecmult_multi_var call, ecmult_impl.h:822-867)."""
        import threading
        sc = _u8(sc); pt_xy = _u8(pt_xy); off = np.ascontiguousarray(offsets, dtype=np.uint64); k = off.size - 1
        n = int(off[-1]) if off.size else 0
        g_sc = None if g_sc is None else _u8(g_sc); pt_inf = None if pt_inf is None else _u8(pt_inf)
        _need("ecmult_multi_many_group sc", sc, 32 * n); _need("ecmult_multi_many_group pt_xy", pt_xy, 64 * n)
        if g_sc is not None: _need("ecmult_multi_many_group g_sc", g_sc, 32 * k)
        if pt_inf is not None: _need("ecmult_multi_many_group pt_inf", pt_inf, n)
        if k > 0 and (int(off[0]) != 0 or np.any(off[1:] < off[:-1])):
            raise S2KError("ecmult_multi_many_group failed: offsets must start at 0 and not decrease")
        from .parallel import shard_sums
        m = len(self)
        cut = shard_sums(off, m)                 # member i takes sums [cut[i], cut[i + 1])
        r = np.zeros((max(k, 0), 64), np.uint8); inf = np.zeros(max(k, 0), np.int32)
        errs = [None] * m

        def run(i):
            a, b = cut[i], cut[i + 1]
            if b <= a: return
            t0, t1 = int(off[a]), int(off[b])
            try:
                xy, fl = self.engine(i).ecmult_multi_many(sc.reshape(-1)[32 * t0:32 * t1], pt_xy.reshape(-1)[64 * t0:64 * t1], off[a:b + 1] - off[a],
                                                          None if g_sc is None else g_sc.reshape(-1)[32 * a:32 * b], None if pt_inf is None else pt_inf.reshape(-1)[t0:t1])
                r[a:b] = xy; inf[a:b] = fl
            except Exception as ex:                  # (reported by the calling thread)
                errs[i] = ex
        ts = [threading.Thread(target=run, args=(i,)) for i in range(m)]
        for t in ts: t.start()
        for t in ts: t.join()
        for ex in errs:
            if ex is not None: raise ex
        return r, inf

    def ecmult_multi_dev(self, sc_list, pt_list, g_sc_dev0=None, inf_list=None):
        """per engine: torch uint8 tensors resident on that engine's GPU (sc (n_i,32), pt (n_i,64)); returns (xy bytes, inf)"""
        k = len(self)
        assert len(sc_list) == k and len(pt_list) == k
        vp = ctypes.c_void_p * k
        a = vp(*[t.data_ptr() for t in sc_list]); b = vp(*[t.data_ptr() for t in pt_list])
        c = None if inf_list is None else vp(*[t.data_ptr() for t in inf_list])
        cnt = (ctypes.c_size_t * k)(*[t.numel() // 32 for t in sc_list])
        r = np.zeros(64, np.uint8); inf = np.zeros(1, np.int32)
        self._check(self._lib.s2k_ecmult_multi_group_dev(self._h, _p(r), _p(inf), _dp(g_sc_dev0), a, b, c, cnt), "s2k_ecmult_multi_group_dev")
        return r, int(inf[0])
