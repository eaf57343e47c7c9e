"""What a batch must look like before it can show a wrong stride or a dropped offset in the host code that places an item in a batch
(csrc/engine_lanes.h: lanes_run; csrc/engine_core.hip: group_by_items and the `_group` lambdas).  A group hands engine i the items
[n*i/k, n*(i+1)/k), a launch loop hands launch j the items [L*j, L*(j+1)): code that forgot `+ lo` or `+ i0` on one array reads row t where
it should read row b + t.  The batches of the family tests are cut cyclically from pools of 200 items, so such code goes unseen when b is
a multiple of the pool's period, or when the rows at t and b + t happen to agree.  check() asserts, on the test's own inputs and before
the engine is called, that neither is the case.  Pure Python and numpy: it runs without a GPU."""
import numpy as np


def share_starts(n, k):
    """the non-zero starts of the shares of n items over k engines (group_share: lo = n * i / k)"""
    return sorted({n * i // k for i in range(1, k)} - {0, n})


def launch_starts(n, lanes):
    """the non-zero starts of the launches of n items under a cap of `lanes` per launch"""
    return list(range(lanes, n, lanes))


def _rows(a, n):
    """n rows of equal width; a list of byte strings of several lengths (DER signatures): each padded, behind its length"""
    if isinstance(a, (list, tuple)):
        w = max(len(x) for x in a)
        a = np.frombuffer(b"".join(bytes([len(x)]) + bytes(x) + bytes(w - len(x)) for x in a), np.uint8)
    return np.ascontiguousarray(a).reshape(n, -1)


def check(what, bounds, arrays, verdicts, period=None, both=True, fixed=()):
    """bounds: the boundaries b of the split.  arrays: {name: array of n rows} that move with the item.  verdicts: the expected verdicts
    (one array, or several that are checked one by one).  period: after how many rows the batch repeats itself, if it does.
    fixed: names of arrays whose rows are the same for every item by construction of the call (nothing to see there).
    * no boundary is a multiple of the period;
    * for every boundary b the items at t and b + t differ for every t among the first 64 positions, and in every array some row of
      an item that must read 1 differs from the row a dropped offset would read in its place (then that item reads 0: seen);
    * every part between two boundaries holds both verdicts (both=False: the batch is too small for that)."""
    verdicts = [np.asarray(v) for v in (verdicts if isinstance(verdicts, (list, tuple)) else [verdicts])]
    n = verdicts[0].size
    rows = {k: _rows(a, n) for k, a in arrays.items()}
    assert all(0 < b < n for b in bounds), (what, bounds, n)
    for b in bounds:
        assert period is None or b % period, (what, "boundary is a multiple of the pool's period", b, period)
        m = min(64, n - b)
        same = np.ones(m, bool)
        for k, a in rows.items():
            d = (a[:m] != a[b:b + m]).any(axis=1)
            same &= ~d
            if k not in fixed:
                for v in verdicts:
                    assert (d & (v[b:b + m] == 1)).any() or not (v[b:b + m] == 1).any(), (what, "rows at t and b + t agree wherever the verdict is 1", k, b)
        assert not same.any(), (what, "items at t and b + t are the same", b, np.flatnonzero(same)[:4])
    if both:
        cuts = [0] + list(bounds) + [n]
        for lo, hi in zip(cuts, cuts[1:]):
            for v in verdicts:
                assert 0 < v[lo:hi].sum() < hi - lo, (what, "a part holds one verdict only", lo, hi)
