"""The contract of labsort_kth_device (include/labsort.h) as a numpy model, shared by test_kth_model.py
and test_gpu_kth.py: row r's output is entry k_r - 1 of the stable ascending sort of the row's
(u(key), position) pairs.  Two forms: by_sort takes the column from rowsort_model.expected (the
whole rows sorted), by_partition finds the same in O(cols) per row with np.partition and the tie
rank.  Arrays are words (uint16 for "bf16" / "f16", uint32 otherwise); kind is a key of ls.KEY; k is
an int or one value per row.  Nothing here calls the library."""
import numpy as np

import rowsort_model as R


def ks_of(k, rows):
    """k as one value per row."""
    ks = np.broadcast_to(np.asarray(k, dtype=np.int64), (rows,))
    return ks


def clamp(k, cols):
    """What the device makes of a k outside [1, cols], and which rows that concerns.  The device reads
    uint32 words: a negative int32 is a large k."""
    k = np.asarray(k, dtype=np.int64) & 0xFFFFFFFF
    return np.clip(k, 1, cols), (k < 1) | (k > cols)


def by_sort(x, k, largest, kind):
    """(keys, positions), one per row: column k_r - 1 of the rows sorted."""
    rows, cols = x.shape
    ks = ks_of(k, rows)
    assert bool(((ks >= 1) & (ks <= cols)).all())
    ek, ei = R.expected(x, largest, kind)
    r = np.arange(rows)
    return ek[r, ks - 1].copy(), ei[r, ks - 1].astype(np.uint32)


def by_partition(x, k, largest, kind):
    """The same without sorting: the k-th image by np.partition, the keys below it counted, and the
    (k - count_below)-th occurrence of the image in position order."""
    rows, cols = x.shape
    ks = ks_of(k, rows)
    assert bool(((ks >= 1) & (ks <= cols)).all())
    u = R.u_of(x, kind, largest)
    keys = np.empty(rows, dtype=x.dtype)
    pos = np.empty(rows, dtype=np.uint32)
    for r in range(rows):
        kk = int(ks[r])
        t = np.partition(u[r], kk - 1)[kk - 1]
        below = int(np.count_nonzero(u[r] < t))
        at = np.flatnonzero(u[r] == t)[kk - below - 1]
        keys[r], pos[r] = x[r, at], at
    return keys, pos


def assert_result(got_k, got_i, want_k, want_i, kind, msg=""):
    """Keys by rowsort_model.assert_keys (a NaN only has to be a NaN), positions exactly."""
    R.assert_keys(np.asarray(got_k).reshape(1, -1), np.asarray(want_k).reshape(1, -1), kind, msg)
    if got_i is not None:
        np.testing.assert_array_equal(np.asarray(got_i, dtype=np.uint32), want_i, err_msg=f"positions {msg}")
