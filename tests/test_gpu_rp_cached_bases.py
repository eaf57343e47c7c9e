"""GPU parity for the per-slot ring-base chain and is-square flag of the generator-table cache (k_rp_prologue skips rp_pp_bases and the
square root for a proof whose generator has a table; a ring of such a proof that the shared form hands back gets its base records from
the slot, k_rp_handback_bases, before k_rp_rings reads them), against the reference compiled here (oracle/_ref).

One pool of 130 proofs cycles through four kinds, so that every prefix mixes them inside its wavefronts:
  served    valid proofs under H (table cached): 64-bit, short (2 rings, last ring of size 2), exponents 0, 3 and 18, a min_value;
  crafted   proofs under H that leave the shared form: suspect rings and exceptional additions (tests/test_gpu_rangeproof_adversarial.py's
            inputs) -- the general form then works on the SLOT's records, for them and for the live neighbours in their wavefronts;
  uncached  valid proofs under a generator without a table (exponent 2): the unchanged per-proof path, ws.bases / ws.dbases;
  broken    a truncated proof and a proof with trailing bytes.
Batches: the first 1, 63, 65 and 130 of the pool plus one proof of every kind alone, with S2K_OPT_RP_SPLIT 0 and 1.
And proofs signed under -H (the other value of the is-square flag: H's y is not a square, -H's is): with -H cached they are accepted and
served by the shared form."""
import numpy as np
import pytest

from tests.adversarial import Crafter
from tests.refapi import GENERATOR_H, P
from tests.test_gpu_rangeproof_adversarial import _crafted

pytestmark = pytest.mark.gpu
GH = np.frombuffer(GENERATOR_H, np.uint8)
NEG_H = GENERATOR_H[:32] + (P - int.from_bytes(GENERATOR_H[32:], "big")).to_bytes(32, "big")
KINDS = ("served", "crafted", "served_exp", "uncached", "broken")


@pytest.fixture(scope="module")
def eng():
    from secp256k1_zkp_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(ref):
    """(C, P, G, kinds, crafted kinds, expected results / min / max of the reference): built and verified once"""
    rng = np.random.default_rng(4100)
    served = []
    for bits, exp, mn in ((64, 0, 0), (3, 0, 0), (7, 0, 0), (52, 0, 9), (3, 0, 5)):
        c, p, g, _ = ref.make_rangeproofs(6, rng, min_bits=bits, exp=exp, min_value=mn)
        served += [(c[i].tobytes(), p[i]) for i in range(6)]
    served_exp = []
    for bits, exp, mn in ((50, 3, 0), (3, 18, 0), (3, 3, 0), (20, 7, 11), (32, 1, 0)):
        c, p, g, _ = ref.make_rangeproofs(6, rng, min_bits=bits, exp=exp, min_value=mn)
        served_exp += [(c[i].tobytes(), p[i]) for i in range(6)]
    g2 = ref.rand_point(rng)
    c, p, g, _ = ref.make_rangeproofs(26, rng, min_bits=20, exp=2, gens64=np.tile(np.frombuffer(g2, np.uint8), (26, 1)))
    uncached = [(c[i].tobytes(), p[i]) for i in range(26)]
    crafted = _crafted(ref, rng)
    order = {"inf": 0, "rinf": 1, "x": 2, "dbl": 3}
    by_kind = {k: [it for it in crafted if it[0] == k] for k in order}
    crafted = [by_kind[k][i] for i in range(max(map(len, by_kind.values()))) for k in order if i < len(by_kind[k])]      # round robin over the kinds
    n = 130
    C = np.zeros((n, 33), np.uint8); Pl = [None] * n; G = np.tile(GH, (n, 1)); kinds = [None] * n; ckind = [None] * n
    for i in range(n):
        k, t = KINDS[i % 5], i // 5
        kinds[i] = k
        if k == "served":
            c, p = served[t % len(served)]
        elif k == "served_exp":
            c, p = served_exp[t % len(served_exp)]
        elif k == "crafted":
            ckind[i], c, p = crafted[t % len(crafted)]
        elif k == "uncached":
            c, p = uncached[t]; G[i] = np.frombuffer(g2, np.uint8)
        else:
            c, p = served[(t + 1) % len(served)]
            p = p[:-1] if t % 2 == 0 else p + b"\x00"
        C[i] = np.frombuffer(c, np.uint8); Pl[i] = p
    want = ref.rangeproof_verify_many(C, Pl, G, threads=8)
    res = want[0]
    assert all(res[i] == 1 for i in range(n) if kinds[i] in ("served", "served_exp", "uncached") or ckind[i] == "dbl")
    assert not any(res[i] for i in range(n) if kinds[i] == "broken" or ckind[i] in ("inf", "x", "rinf"))
    return C, Pl, G, kinds, ckind, want, g2


def _check(eng, pool, idx):
    C, Pl, G, kinds, ckind, want, _ = pool
    res, mn, mx = eng.rangeproof_verify_batch(C[idx], [Pl[i] for i in idx], G[idx])
    assert np.array_equal(res, want[0][idx]), [(i, kinds[i], ckind[i]) for i in np.asarray(idx)[res != want[0][idx]]]
    assert np.array_equal(mn, want[1][idx]) and np.array_equal(mx, want[2][idx])
    return eng.rp_handback()


@pytest.mark.parametrize("split", (0, 1))
def test_mixed_batches_read_the_slot_chain(eng, pool, split):
    from secp256k1_zkp_amd import Engine
    kinds, ckind, g2 = pool[3], pool[4], pool[6]
    eng.set_option(Engine.OPT_RP_SPLIT, split)
    eng.cache_generator(GENERATOR_H)
    assert eng.generator_cached(GENERATOR_H) and not eng.generator_cached(g2)
    for n in (63, 65, 130):
        hb = _check(eng, pool, np.arange(n))
        assert hb[0] > 0 and hb[2] > 0 and hb[3] > 0, (n, hb)         # shared form used; suspect rings and exceptional additions went back
        assert hb[1] > hb[2] + hb[3], (n, hb)                         # and the general form also had the uncached generator's rings
    # the first proof of the pool alone, then one of every kind alone
    firsts = [0] + [kinds.index(k) for k in KINDS[1:]] + [ckind.index(k) for k in ("inf", "x", "rinf", "dbl")]
    for i in firsts:
        hb = _check(eng, pool, np.array([i]))
        if kinds[i] in ("served", "served_exp"):
            assert hb[0] > 0 and hb[1] == 0, (i, hb)
        if kinds[i] == "uncached":
            assert hb[0] == 0 and hb[1] > 0, (i, hb)
        if ckind[i] in ("inf", "x"):
            assert hb[0] > 0 and hb[2] > 0 and hb[1] >= hb[2], (i, ckind[i], hb)
        if ckind[i] in ("rinf", "dbl"):
            assert hb[0] > 0 and hb[3] > 0 and hb[1] >= hb[3], (i, ckind[i], hb)


def test_generator_with_the_other_square_flag(eng, ref):
    """-H: exactly one of y and -y is a square, so the flag a slot keeps for -H is the opposite of H's (the message hash carries it: H's
    y is NOT a square, -H's is), and its chain starts at +H"""
    from secp256k1_zkp_amd import Engine
    rng = np.random.default_rng(4101)
    euler = [pow(int.from_bytes(g[32:], "big"), (P - 1) // 2, P) for g in (GENERATOR_H, NEG_H)]
    assert euler == [P - 1, 1]
    gn = np.tile(np.frombuffer(NEG_H, np.uint8), (65, 1))
    parts = [ref.make_rangeproofs(k, rng, min_bits=b, exp=e, gens64=gn[:k]) for k, b, e in ((40, 64, 0), (15, 3, 0), (10, 30, 4))]
    C = np.concatenate([x[0] for x in parts]); Pl = sum((x[1] for x in parts), []); G = gn
    want = ref.rangeproof_verify_many(C, Pl, G, threads=8)
    assert want[0].all()
    eng.set_option(Engine.OPT_RP_SPLIT, 1)
    try:
        eng.cache_generator(NEG_H)
        assert eng.generator_cached(NEG_H)
        res, mn, mx = eng.rangeproof_verify_batch(C, Pl, G)
        hb = eng.rp_handback()
        assert np.array_equal(res, want[0]) and np.array_equal(mn, want[1]) and np.array_equal(mx, want[2])
        assert hb[0] > 0 and hb[1] == 0 and hb[2] == 0 and hb[3] == 0, hb          # served by the shared form, nothing through the general one
        # signed under -H but presented with H: the flag byte and the bases differ, the reference rejects and so does the engine
        GHn = np.tile(GH, (65, 1))
        want2 = ref.rangeproof_verify_many(C, Pl, GHn, threads=8)
        res2, _, _ = eng.rangeproof_verify_batch(C, Pl, GHn)
        assert not want2[0].any() and np.array_equal(res2, want2[0])
    finally:
        eng.cache_generator(GENERATOR_H)                                           # (H keeps its table for whoever comes next on this device)
