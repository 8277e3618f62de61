"""tests/topk_mask_model.py against itself and against a plain Python loop: the two forms of the
contract (the first k positions of the rows sorted; the threshold pair (T, P) and the elementwise
test) give the same filtered words and the same mask, for all five kinds and both directions, on rows
with ties at the threshold, all-equal and all-NaN rows, both zeros, k = 1 and k = cols, and a k per row
with entries that the device would clamp.  No library call."""
import numpy as np
import pytest

import kth_model as K
import rowsort_model as R
import topk_mask_model as TM

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", R.KINDS)
FLOATS = ("f32", "bf16", "f16")
ZEROS = {"f32": (0x80000000, 0x00000000), "bf16": (0x8000, 0x0000), "f16": (0x8000, 0x0000)}  # (-0.0, +0.0)


def by_loop(x, k, largest, kind, fill):
    """The contract word for word: sort the row's (u, position) pairs, keep the first k."""
    rows, cols = x.shape
    ks = K.ks_of(k, rows)
    u = R.u_of(x, kind, largest)
    out = np.full(x.shape, fill, dtype=x.dtype)
    mask = np.zeros(x.shape, dtype=np.uint8)
    for r in range(rows):
        pairs = sorted((int(u[r, i]), i) for i in range(cols))
        for _, i in pairs[:int(ks[r])]:
            out[r, i] = x[r, i]
            mask[r, i] = 1
    return out, mask


def agree(x, k, largest, kind, fill=None):
    fill = TM.default_fill(kind, largest) if fill is None else fill
    a = TM.by_sort(x, k, largest, kind, fill)
    b = TM.by_threshold(x, k, largest, kind, fill)
    c = by_loop(x, k, largest, kind, fill)
    for other in (b, c):
        np.testing.assert_array_equal(a[0], other[0])
        np.testing.assert_array_equal(a[1], other[1])
    ks = K.ks_of(k, x.shape[0])
    np.testing.assert_array_equal(a[1].sum(axis=1), ks)  # exactly k_r kept
    assert a[0].dtype == x.dtype and a[1].dtype == np.uint8
    return a


@KINDS
@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("gen", ["mixed", "ties"])
def test_forms_agree(kind, largest, gen):
    for rows, cols in ((4, 1), (3, 2), (5, 67), (3, 300)):
        x, _ = R.case(kind, rows, cols, gen)
        for k in (1, (cols + 1) // 2, cols):
            agree(x, k, largest, kind)
        agree(x, np.random.default_rng(cols).integers(1, cols + 1, size=rows), largest, kind)


@KINDS
@pytest.mark.parametrize("largest", BOTH)
def test_all_equal_rows(kind, largest):
    """Every key is a tie of the threshold: the first k positions are kept."""
    cols = 41
    x = np.full((3, cols), R.random_words((1,), 7, kind)[0], dtype=R.wdtype(kind))
    for k in (1, 20, cols):
        _, mask = agree(x, k, largest, kind)
        assert bool((mask[:, :k] == 1).all()) and bool((mask[:, k:] == 0).all())


@pytest.mark.parametrize("kind", FLOATS)
@pytest.mark.parametrize("largest", BOTH)
def test_all_nan_rows(kind, largest):
    """NaNs of several payloads and both signs are one value."""
    cols = 37
    nans = np.array([R.nan_word(kind), 0x7FC00000 if kind == "f32" else 0x7FC1, 0xFFFFFFFF if kind == "f32" else 0xFFFF])
    x = nans[np.random.default_rng(3).integers(0, 3, size=(2, cols))].astype(R.wdtype(kind))
    for k in (1, 9, cols):
        _, mask = agree(x, k, largest, kind)
        assert bool((mask[:, :k] == 1).all()) and bool((mask[:, k:] == 0).all())


@pytest.mark.parametrize("kind", FLOATS)
def test_both_zeros(kind):
    """-0.0 < +0.0: ascending the negative zeros go first, descending the positive ones."""
    neg, pos = ZEROS[kind]
    x = np.array([[pos, neg, pos, neg, neg, pos]], dtype=R.wdtype(kind))
    _, mask = agree(x, 3, False, kind)
    assert mask.tolist() == [[0, 1, 0, 1, 1, 0]]
    _, mask = agree(x, 3, True, kind)
    assert mask.tolist() == [[1, 0, 1, 0, 0, 1]]
    _, mask = agree(x, 4, False, kind)
    assert mask.tolist() == [[1, 1, 0, 1, 1, 0]]
    _, mask = agree(x, 2, True, kind)
    assert mask.tolist() == [[1, 0, 1, 0, 0, 0]]


@KINDS
def test_ties_at_the_threshold(kind):
    """Of the threshold's ties the lowest positions survive, whatever the fill."""
    lo, mid, hi = {"u32": (5, 9, 0x80000001), "i32": (0xFFFFFFFE, 0, 3), "f32": (0xBF800000, 0x40000000, 0x40400000),
                   "bf16": (0xBF80, 0x4000, 0x4040), "f16": (0xBC00, 0x4000, 0x4200)}[kind]  # (-2 0 3; -1.0 2.0 3.0)
    x = np.array([[mid, hi, mid, lo, mid, hi, mid]], dtype=R.wdtype(kind))
    _, mask = agree(x, 3, False, kind)  # lo and the first two mids
    assert mask.tolist() == [[1, 0, 1, 1, 0, 0, 0]]
    out, mask = agree(x, 4, True, kind, fill=int(mid))  # both his and the first two mids; the fill equals a key
    assert mask.tolist() == [[1, 1, 1, 0, 0, 1, 0]]
    assert int(out[0, 4]) == int(mid) and int(mask[0, 4]) == 0


@KINDS
def test_clamped_k_per_row(kind):
    """What the device makes of a k outside [1, cols] (kth_model.clamp), then the model."""
    x, _ = R.case(kind, 5, 67)
    bad = np.array([0, 68, -1, 5, 67])
    ks, which = K.clamp(bad, 67)
    assert ks.tolist() == [1, 67, 67, 5, 67] and which.tolist() == [True, True, True, False, False]
    for largest in BOTH:
        _, mask = agree(x, ks, largest, kind)
        assert mask.sum(axis=1).tolist() == [1, 67, 67, 5, 67]


def test_default_fill_is_the_worst_key():
    for kind in R.KINDS:
        for largest in BOTH:
            f = np.array([[TM.default_fill(kind, largest)]], dtype=R.wdtype(kind))
            x = R.random_words((1, 200), 5, kind)
            if kind in FLOATS:  # (NaNs are larger than +inf)
                u = R.u_of(x, kind, False)
                x = x[u < R.u_of(np.array([[R.nan_word(kind)]], dtype=R.wdtype(kind)), kind, False)[0, 0]].reshape(1, -1)
            assert bool((R.u_of(f, kind, largest)[0, 0] >= R.u_of(x, kind, largest)).all())
