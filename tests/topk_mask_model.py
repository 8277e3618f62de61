"""The contract of labsort_topk_mask_device (include/labsort.h) as a numpy model, shared by
test_topk_mask_model.py and test_gpu_topk_mask.py: element i of row r is kept iff (u(key_i), i) is among
the first k_r entries of the stable ascending sort of the row's (u, position) pairs.  Two forms: by_sort
keeps the first k_r positions of rowsort_model.expected, by_threshold takes kth_model.by_partition's
(T, P) and tests every element against it.  Both return (filtered words, mask): a kept element keeps
its word (for the float kinds a NaN stays some NaN: rowsort_model.assert_keys), every other element is
`fill`.  Arrays are words (uint16 for "bf16" / "f16", uint32 otherwise); kind is a key of ls.KEY; k is an
int or one value per row, inside [1, cols] (kth_model.clamp first where it is not).  Nothing here calls
the library."""
import numpy as np

import kth_model as K
import rowsort_model as R


def by_sort(x, k, largest, kind, fill):
    rows, cols = x.shape
    ks = K.ks_of(k, rows)
    assert bool(((ks >= 1) & (ks <= cols)).all())
    _, ei = R.expected(x, largest, kind)
    mask = np.zeros((rows, cols), dtype=np.uint8)
    for r in range(rows):
        mask[r, ei[r, :int(ks[r])].astype(np.int64)] = 1
    return np.where(mask != 0, x, R.wdtype(kind)(fill)).astype(x.dtype), mask


def by_threshold(x, k, largest, kind, fill):
    rows, cols = x.shape
    tk, tp = K.by_partition(x, k, largest, kind)
    u = R.u_of(x, kind, largest)
    ut = R.u_of(tk.reshape(rows, 1), kind, largest)
    at = np.arange(cols, dtype=np.int64)[None, :]
    keep = (u < ut) | ((u == ut) & (at <= tp.astype(np.int64)[:, None]))
    return np.where(keep, x, R.wdtype(kind)(fill)).astype(x.dtype), keep.astype(np.uint8)


def default_fill(kind, largest):
    """The worst word for the direction: -inf / +inf, the integer order's first / last."""
    lo, hi = {"u32": (0, 0xFFFFFFFF), "i32": (0x80000000, 0x7FFFFFFF), "f32": (0xFF800000, 0x7F800000),
              "bf16": (0xFF80, 0x7F80), "f16": (0xFC00, 0x7C00)}[kind]
    return lo if largest else hi


def assert_result(got_keys, got_mask, want_keys, want_mask, kind, msg=""):
    """Every output that was asked for: keys by rowsort_model.assert_keys, the mask byte for byte."""
    if got_mask is not None:
        np.testing.assert_array_equal(np.asarray(got_mask, dtype=np.uint8), want_mask, err_msg=f"mask {msg}")
    if got_keys is not None:
        R.assert_keys(got_keys, want_keys, kind, msg)
