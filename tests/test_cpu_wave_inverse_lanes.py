"""The bounds of the lane-distributed uniform inverse (csrc/modinv.h: ds_inverse_words_lanes), on its Python model
(tests/waveinv_lanes_model.py): nine lanes of limbs, one and a half carry passes, 64-bit wraparound made explicit.  The model asserts
after every operation what the header comment of the device code states -- no column sum leaves the signed 64-bit range or the stated
|S| <= 2^61 + 2^31, every operand of a 32 x 32 + 64 multiply-add fits 32 bits, limbs 0..7 stay in [-3, 2^30 + 2], lane 0 is exact, the
top limb stays below 2^22, lanes above 8 stay zero -- and this test runs it over 2 * 10^4 seeded values per modulus and the edge values.
This test, not the comment, guards the bound."""
import random

import numpy as np
import pytest

from tests import waveinv_lanes_model as M


def edge_values(m):
    return [1, 2, m - 1, m - 2, (m + 1) // 2, (1 << 255) % m, 1 << 30, (1 << 30) - 1, 1 << 240, 0]


@pytest.mark.parametrize("mod", ["p", "n"])
def test_lane_model_bounds_and_results(mod):
    m = M.MODS[mod][0]
    rnd = random.Random(20260 + ord(mod))
    vals = [rnd.randrange(m) for _ in range(20000)] + edge_values(m)
    r = M.run(vals, mod)                            # asserts every range on the way
    for v, x in zip(vals, r.results):
        assert x == (pow(v, -1, m) if v else 0)
    assert int(r.sum_max.max()) <= M.SUM_MAX and int(r.sum_min.min()) >= -M.SUM_MAX
    assert M.SUM_MAX < (1 << 63)


@pytest.mark.parametrize("mod", ["p", "n"])
def test_lane_model_values_are_the_exact_ones(mod):
    """limbs summed = the batches on Python integers (so |d|, |e| < 21 m as for the scalar form), and the early exit -- taken on g with its
    carries rippled through -- leaves at the batch at which g is 0, as the scalar form does"""
    m = M.MODS[mod][0]
    rnd = random.Random(31 + ord(mod))
    vals = [rnd.randrange(m) for _ in range(200)] + edge_values(m)
    r = M.run(vals, mod, record=True)
    for i, v in enumerate(vals):
        exact, g_zero_at = M.exact_batches(v, mod)
        assert g_zero_at is not None
        assert r.batches[i] == max(g_zero_at, M.BATCHES - 4)
        for it in range(int(r.batches[i])):
            f, g, d, e = (M.value_of(a[i]) for a in r.states[it])
            assert (f, g, d, e) == exact[it]
            assert abs(d) < (it + 2) * m and abs(e) < (it + 2) * m


def test_batch_matrix_rows_are_bounded():
    """|u| + |v| <= 2^30 and |q| + |r| <= 2^30 for any low words (asserted inside batch()): the premise of the column-sum bound"""
    rng = np.random.default_rng(5)
    n = 200000
    f = rng.integers(0, 1 << 32, n, dtype=np.int64) | 1
    g = rng.integers(0, 1 << 32, n, dtype=np.int64)
    zeta = rng.integers(-40, 40, n, dtype=np.int64)
    M.batch(zeta, f, g)


def test_carry_step_at_the_stated_bound():
    """the carry step of the model on column sums at +-SUM_MAX and around every edge of the lo / mid / top split (the rows the device is
    held to in tests/test_gpu_wave_inverse_lanes.py): every register width holds (asserted inside carry()), the limbs that come out
    stay in [-3, 2^30 + 2] and reach both ends, and they carry the value of the sums divided by 2^30"""
    from tests.test_gpu_wave_inverse_lanes import carry_edge_rows
    rows = carry_edge_rows()
    assert int(rows.max()) == M.SUM_MAX and int(rows.min()) == -M.SUM_MAX
    out = M.carry(rows)
    assert int(out[:, :8].min()) == M.LIMB_LO and int(out[:, :8].max()) == M.LIMB_HI
    for r, o in zip(rows[::37], out[::37]):
        assert M.value_of(o) == (M.value_of(r) - (int(r[0]) & M.MASK)) >> M.BITS
