"""tests/kth_model.py against itself (CPU): the two forms of the k-th key's contract, by sorting whole
rows and by np.partition plus the tie rank, agree on small arrays with heavy ties and NaNs, for every
kind, both directions, one k and a k per row."""
import numpy as np
import pytest

import kth_model as K
import rowsort_model as R

KINDS = pytest.mark.parametrize("kind", R.KINDS)


@KINDS
@pytest.mark.parametrize("gen", ["ties", "planted", "random"])
def test_forms_agree(kind, gen):
    for rows, cols in ((1, 1), (3, 2), (4, 17), (5, 200), (2, 1000)):
        x = {"ties": R.tie_words, "planted": R.planted_words, "random": R.random_words}[gen]((rows, cols), 0x4B01 + cols, kind)
        x = np.ascontiguousarray(x, dtype=R.wdtype(kind))
        rng = np.random.default_rng(cols)
        for largest in (False, True):
            for k in (1, (cols + 1) // 2, cols, rng.integers(1, cols + 1, size=rows)):
                k1, i1 = K.by_sort(x, k, largest, kind)
                k2, i2 = K.by_partition(x, k, largest, kind)
                np.testing.assert_array_equal(k1, k2)
                np.testing.assert_array_equal(i1, i2)
                np.testing.assert_array_equal(x[np.arange(rows), i1.astype(np.int64)], k1)


@KINDS
def test_tie_rule_and_nans(kind):
    """All keys equal: the k-th is at position k - 1 in both directions.  NaNs of several payloads are
    one value, the largest: ascending they fill the last ranks in position order, descending the first."""
    cols = 37
    x = np.full((1, cols), R.random_words((1,), 3, kind)[0], dtype=R.wdtype(kind))
    for largest in (False, True):
        for k in (1, 5, cols):
            assert int(K.by_partition(x, k, largest, kind)[1][0]) == k - 1
            assert int(K.by_sort(x, k, largest, kind)[1][0]) == k - 1
    if kind in ("f32", "bf16", "f16"):
        y = R.tie_words((1, 400), 0x4B02, kind)
        y = np.ascontiguousarray(y, dtype=R.wdtype(kind))
        nan = np.flatnonzero(R.u_of(y, kind)[0] == R.u_of(y, kind).max())
        assert nan.size > 3
        for j in (1, 2, nan.size):
            assert int(K.by_partition(y, j, True, kind)[1][0]) == nan[j - 1]
            assert int(K.by_partition(y, 400 - nan.size + j, False, kind)[1][0]) == nan[j - 1]


def test_clamp():
    k, bad = K.clamp([0, 1, 7, 8, -3, 1 << 31], 7)
    np.testing.assert_array_equal(k, [1, 1, 7, 7, 7, 7])  # (-3 is the word 0xFFFFFFFD)
    np.testing.assert_array_equal(bad, [True, False, False, True, True, True])
