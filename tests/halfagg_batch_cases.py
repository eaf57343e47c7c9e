"""The cases of the batch half-aggregate tests, from tests/golden/halfagg_batch_vectors.json (written by
tests/golden/make_halfagg_batch_golden.py from the reference's answers): every aggregate and tampered copy as one Case, the batch
shapes both tiers run, and the packing into the back-to-back arrays of the C ABI.  Loaded once per process and never changed."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MM_MAX_TERMS = 8192                      # engine_msm_many.hip: aggregates of more than 4 096 signatures take the single-aggregate path


class Case:
    """keys[0]: n*32 serialised keys, keys[1]: n*64 key objects; sigs only where the aggregate is the reference's own"""

    def __init__(self, name, n, pks, objs, msgs, agg, result, sigs=None):
        self.name, self.n, self.keys, self.msgs, self.agg, self.result, self.sigs = name, n, (pks, objs), msgs, agg, result, sigs


def _apply(rec, t):
    f = {"pks": bytearray.fromhex(rec["pks"]), "msgs": bytearray.fromhex(rec["msgs"]), "agg": bytearray.fromhex(rec["agg"]), "objs": bytearray.fromhex(rec["objs"])}
    for field, off, hx in t["patches"]:
        if field == "agg_len":
            f["agg"] = f["agg"][:off] + bytes(max(0, off - len(f["agg"])))
        else:
            b = bytes.fromhex(hx); f[field][off:off + len(b)] = b
    for k, hx in t.get("objs", []):
        f["objs"][64 * k:64 * k + 64] = bytes.fromhex(hx)
    return bytes(f["pks"]), bytes(f["objs"]), bytes(f["msgs"]), bytes(f["agg"])


@functools.lru_cache(None)
def golden():
    return json.load(open(os.path.join(HERE, "golden", "halfagg_batch_vectors.json")))


@functools.lru_cache(None)
def cases():
    """every recorded aggregate (name 'n=<n>') and tampered copy (name 'n=<n> <what>'), in file order"""
    out = []
    for rec in golden()["aggregates"]:
        n = rec["n"]
        out.append(Case(f"n={n}", n, bytes.fromhex(rec["pks"]), bytes.fromhex(rec["objs"]), bytes.fromhex(rec["msgs"]), bytes.fromhex(rec["agg"]), rec["result"],
                        bytes.fromhex(rec["sigs"])))
        for t in rec["tampered"]:
            out.append(Case(f"n={n} {t['name']}", n, *_apply(rec, t), t["result"]))
    return tuple(out)


def good():
    return [c for c in cases() if c.sigs is not None]


@functools.lru_cache(None)
def repeated():
    """the aggregate above the many-sums limit: one triple 4 097 times with the reference's s"""
    r = golden()["repeated"]; m = r["count"]
    sig = bytes.fromhex(r["sig"])
    return Case(f"n={m} repeated", m, bytes.fromhex(r["pk"]) * m, bytes.fromhex(r["obj"]) * m, bytes.fromhex(r["msg"]) * m, sig[:32] * m + bytes.fromhex(r["s"]), r["result"],
                sig * m)


def shuffled():
    """every case once, sizes in shuffled order; the running item count in front of an aggregate is odd for some and even for others"""
    order = np.random.default_rng(7).permutation(len(cases()))
    batch = [cases()[i] for i in order]
    firsts = np.cumsum([0] + [c.n for c in batch])[:-1]
    assert {int(f) & 1 for f, c in zip(firsts, batch) if c.n} == {0, 1}
    return batch


def of_count(m):
    """m aggregates cycling through the cases from a case-dependent start (1, 63, 64, 65: a wavefront edge of the chain kernel)"""
    cs = cases()
    return [cs[(5 * m + 3 * i) % len(cs)] for i in range(m)]


def owns_lane(c):
    """the chain kernel gives the aggregate a lane: at least one full block to hash and the right length"""
    return c.n >= 1 and len(c.agg) == 32 * (c.n + 1)


def with_lanes(m):
    """m aggregates that EACH own a lane of the chain kernel, accepted and tampered ones of every size in mixed order: exactly m lanes, so
    that 63 / 64 / 65 is one lane short of a wavefront, a full wavefront, and a second workgroup with one lane; the sizes differ, so the
    lane -> aggregate permutation (descending by size) is not the identity"""
    cs = [c for c in cases() if owns_lane(c)]
    batch = [cs[(7 * i + m) % len(cs)] for i in range(m)]
    assert all(owns_lane(c) for c in batch) and len({c.n for c in batch}) >= min(m, 5) and (m < 8 or any(c.result for c in batch))
    return batch


def good_with_lanes(m):
    """the same for the aggregation calls: m of the reference's own aggregates with n >= 1, sizes in mixed order"""
    g = [c for c in good() if c.n >= 1]
    batch = [g[(3 * i + m) % len(g)] for i in range(m)]
    assert [c.n for c in batch] != sorted((c.n for c in batch), reverse=True) or m == 1
    return batch


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def offsets(counts):
    off = np.zeros(len(counts) + 1, np.uint64)
    off[1:] = np.cumsum(np.array(counts, np.uint64), dtype=np.uint64)
    return off


def pack_verify(batch, pk_format):
    """-> keys, msgs, item_off, aggsigs, aggsig_off (numpy), expected verdicts"""
    return (_u8(b"".join(c.keys[pk_format] for c in batch)), _u8(b"".join(c.msgs for c in batch)), offsets([c.n for c in batch]), _u8(b"".join(c.agg for c in batch)),
            offsets([len(c.agg) for c in batch]), [c.result for c in batch])


def pack_inc(batch, pk_format, before, prefix_aggs):
    """-> aggsigs_in, n_before, keys, msgs, new_sigs, item_off for aggregates that already hold before[k] signatures (prefix_aggs[k]:
    the 32 (before[k] + 1) bytes they hold).  The expected output is the reference's FULL aggregate, c.agg: by main_impl.h:43-99
    inc_aggregate(aggregate(first a), rest) == aggregate(all), byte for byte."""
    assert all(len(a) == 32 * (b + 1) and b <= c.n for a, b, c in zip(prefix_aggs, before, batch))
    return (_u8(b"".join(prefix_aggs)), np.array(list(before) + [0], np.uint64), _u8(b"".join(c.keys[pk_format] for c in batch)), _u8(b"".join(c.msgs for c in batch)),
            _u8(b"".join(c.sigs[64 * b:] for c, b in zip(batch, before))), offsets([c.n for c in batch]))


def splits(n):
    return sorted({0, min(1, n), max(n - 1, 0), n})


def out_slices(item_off, out):
    n = len(item_off) - 1
    return [bytes(out[32 * (int(item_off[k]) + k):32 * (int(item_off[k + 1]) + k + 1)]) for k in range(n)]


# ---- the checks both tiers run; `verify` and `inc` are the tier's way of making the call -------------------------------------------------
#   verify(keys, pk_format, msgs, item_off, aggsigs, aggsig_off) -> verdicts (n_aggs ints)
#   inc(aggsigs_in or None, n_before or None, keys, pk_format, msgs, new_sigs, item_off) -> (verdicts, output bytes); None: plain aggregation
def check_verify(verify, batch, pk_format):
    keys, msgs, item_off, aggs, agg_off, want = pack_verify(batch, pk_format)
    got = [int(x) for x in verify(keys, pk_format, msgs, item_off, aggs, agg_off)]
    assert got == want, [(c.name, g, w) for c, g, w in zip(batch, got, want) if g != w]
    assert 1 in want or len(batch) < 3


def check_aggregate(inc, batch, pk_format):
    """plain aggregation against the reference's aggregates, then every split of the incremental form"""
    keys, msgs, item_off = _u8(b"".join(c.keys[pk_format] for c in batch)), _u8(b"".join(c.msgs for c in batch)), offsets([c.n for c in batch])
    res, out = inc(None, None, keys, pk_format, msgs, _u8(b"".join(c.sigs for c in batch)), item_off)
    assert [int(x) for x in res] == [1] * len(batch)
    assert out_slices(item_off, out) == [c.agg for c in batch]
    for s in range(4):
        before = [splits(c.n)[min(s, len(splits(c.n)) - 1)] for c in batch]
        # what the aggregates already hold: the aggregate of the prefix, made by the plain call (checked through the final bytes)
        pk_b = 64 if pk_format else 32
        pre_off = offsets(before)
        pres, pout = inc(None, None, _u8(b"".join(c.keys[pk_format][:pk_b * b] for c, b in zip(batch, before))), pk_format,
                         _u8(b"".join(c.msgs[:32 * b] for c, b in zip(batch, before))), _u8(b"".join(c.sigs[:64 * b] for c, b in zip(batch, before))), pre_off)
        assert [int(x) for x in pres] == [1] * len(batch)
        prefix = [p if b else b"\xff" * 32 for p, b in zip(out_slices(pre_off, pout), before)]      # (n_before = 0: s_old is never read)
        old, nb, keys, msgs, new, item_off = pack_inc(batch, pk_format, before, prefix)
        res, out = inc(old, nb, keys, pk_format, msgs, new, item_off)
        assert [int(x) for x in res] == [1] * len(batch), (s, before)
        assert out_slices(item_off, out) == [c.agg for c in batch], (s, before)


def check_aggregate_refusals(inc, pk_format):
    """a key the reference refuses fails ITS aggregate (zeroed output), in an old and in a new position; the neighbours are the reference's"""
    by = {c.name: c for c in cases()}
    g5, bad5, g2, g16 = by["n=5"], by["n=5 key does not parse"], by["n=2"], by["n=16"]
    spoiled = Case("n=5 refused", 5, bad5.keys[0], bad5.keys[1], g5.msgs, bytes(32 * 6), 0, g5.sigs)
    batch = [g2, spoiled, g16, spoiled, g5]
    for before5 in (0, 5):
        before = [0, before5, 0, before5, 0]
        prefix = [b"\xff" * 32 if not b else g5.agg for b in before]
        old, nb, keys, msgs, new, item_off = pack_inc(batch, pk_format, before, prefix)
        res, out = inc(old, nb, keys, pk_format, msgs, new, item_off)
        assert [int(x) for x in res] == [1, 0, 1, 0, 1]
        assert out_slices(item_off, out) == [c.agg for c in batch]
