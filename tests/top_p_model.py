"""The contract of labsort_top_p_device (include/labsort.h) as a numpy model with Python integers,
shared by test_top_p_model.py and test_gpu_top_p.py.  An element weighs w = min(floor(x 2^40), 2^40), 0
for a set sign bit and for a NaN, taken from the bits; a row's total is W, its fixed-point p is
P = clamp(floor(p 2^32), 1, 2^32), its target t = max(1, ceil(P W / 2^32)); k is the smallest n such
that the weights of the first n entries of the row sorted descending (rowsort_model.expected) reach t,
and the row keeps those n elements; a row with W == 0 is kept whole.  Two forms of the outputs: by_scan
walks the sorted row, by_threshold finds the threshold key without sorting and goes through
topk_mask_model.by_threshold.  Arrays are words (uint16 for "bf16" / "f16", uint32 for "f32").
Nothing here calls the library."""
import numpy as np

import rowsort_model as R
import topk_mask_model as TM

KINDS = ("f32", "bf16", "f16")
FRAC = 40
ONE = 1 << FRAC


def widen(x, kind):
    """The float32 words of the exact float32 values of the words x."""
    x = np.asarray(x)
    if kind == "f32":
        return x.astype(np.uint32)
    if kind == "bf16":
        return x.astype(np.uint32) << np.uint32(16)
    return x.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)  # (exact; a NaN stays a NaN)


def weight(x, kind):
    """uint64 weights of the words x, by integer shifts on the float32 word."""
    b = widen(x, kind).astype(np.uint64)
    e = (b >> np.uint64(23)) & np.uint64(0xFF)
    sig = np.where(e != 0, (b & np.uint64(0x7FFFFF)) | np.uint64(0x800000), b & np.uint64(0x7FFFFF))
    sh = np.maximum(e, np.uint64(1)).astype(np.int64) - 110  # x 2^40 = sig 2^sh
    up = sig << np.clip(sh, 0, 16).astype(np.uint64)
    down = sig >> np.clip(-sh, 0, 63).astype(np.uint64)
    w = np.where(sh >= 0, up, down)
    w = np.where(b >= np.uint64(0x3F800000), np.uint64(ONE), w)  # 1.0 and above, +inf
    return np.where(b > np.uint64(0x7F800000), np.uint64(0), w).astype(np.uint64)  # the sign bit, or a NaN


def fixed_p(p):
    """(P, bad) of one float32 p: bad where p is a NaN or outside (0, 1]."""
    p = float(np.float32(p))
    if p != p or p > 1.0:
        return 1 << 32, True
    if p <= 0.0:
        return 1, True
    return min(max(int(np.floor(p * 4294967296.0)), 1), 1 << 32), False  # (p 2^32 is exact in float64)


def target(P, W):
    return max(1, -((-P * W) >> 32))


def ps_of(p, rows):
    return np.broadcast_to(np.asarray(p, dtype=np.float32), (rows,))


def kept_counts(x, p, kind, exp=None):
    """(k, flagged): k_r per row (int64) and whether the status call reports ERR_ARG.  exp: the rows
    sorted descending (rowsort_model.expected(x, True, kind)) where a test has them."""
    rows, cols = x.shape
    ps = ps_of(p, rows)
    ek, _ = R.expected(x, True, kind) if exp is None else exp
    ks = np.empty(rows, dtype=np.int64)
    flagged = False
    for r in range(rows):
        P, bad = fixed_p(ps[r])
        w = weight(ek[r], kind)
        W = int(w.sum(dtype=np.uint64))  # (< 2^63 for cols <= 2^23)
        flagged |= bad or W == 0
        if W == 0:
            ks[r] = cols
            continue
        run = np.cumsum(w, dtype=np.uint64)
        ks[r] = int(np.searchsorted(run, np.uint64(target(P, W)), side="left")) + 1
    return ks, flagged


def by_scan(x, p, kind, fill, exp=None):
    """(filtered words, mask, k, flagged): the first k_r positions of the sorted row are kept."""
    rows, cols = x.shape
    exp = R.expected(x, True, kind) if exp is None else exp
    ks, flagged = kept_counts(x, p, kind, exp)
    mask = np.zeros((rows, cols), dtype=np.uint8)
    for r in range(rows):
        mask[r, exp[1][r, :int(ks[r])].astype(np.int64)] = 1
    return np.where(mask != 0, x, R.wdtype(kind)(fill)).astype(x.dtype), mask, ks, flagged


def by_threshold(x, p, kind, fill):
    """The same without sorting: per distinct image the count and the mass, the image at which the
    running mass reaches t, ceil(rest / w(T)) of its ties, and topk_mask_model.by_threshold on that k."""
    rows, cols = x.shape
    ps = ps_of(p, rows)
    u = R.u_of(x, kind, True)
    w = weight(x, kind)
    ks = np.empty(rows, dtype=np.int64)
    flagged = False
    for r in range(rows):
        P, bad = fixed_p(ps[r])
        W = int(w[r].sum(dtype=np.uint64))
        flagged |= bad or W == 0
        if W == 0:
            ks[r] = cols
            continue
        t = target(P, W)
        _, first, cnt = np.unique(u[r], return_index=True, return_counts=True)
        wu = w[r][first]  # equal images have equal weights (the NaNs: 0)
        mass = np.cumsum(wu * cnt.astype(np.uint64), dtype=np.uint64)
        i = int(np.searchsorted(mass, np.uint64(t), side="left"))
        below = int(mass[i - 1]) if i else 0
        ks[r] = int(cnt[:i].sum()) + -(-(t - below) // int(wu[i]))
    keys, mask = TM.by_threshold(x, ks, True, kind, fill)
    return keys, mask, ks, flagged


# ---- inputs shared by the CPU and the GPU tests ----

def words_of(q, kind):
    """The words of the finite values q rounded to the kind (to nearest, ties to even)."""
    q = np.asarray(q).astype(np.float32)
    if kind == "f32":
        return q.view(np.uint32)
    if kind == "f16":
        return q.astype(np.float16).view(np.uint16)
    w = q.view(np.uint32)
    return ((w + np.uint32(0x7FFF) + ((w >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def softmax_of(z):
    """The softmax of every row of the float64 logits z."""
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_words(cols, kind, seed, temperature=1.0, rows=2):
    """Rows of softmax(standard normal logits / temperature), computed in float64 and rounded to the kind."""
    return words_of(softmax_of(np.random.default_rng(seed).standard_normal((rows, cols)) / temperature), kind)


def special_rows(kind, cols, seed):
    """Softmax rows with ties, NaNs, values above 1, negatives, zeros and tiny values planted; one row of
    zeros and negatives alone (no mass)."""
    x = softmax_words(cols, kind, seed, rows=4).copy()
    rng = np.random.default_rng(seed + 1)
    one = {"f32": 0x3F800000, "bf16": 0x3F80, "f16": 0x3C00}[kind]
    sign = 0x8000 if R.is16(kind) else 0x80000000
    plant = [R.nan_word(kind), one, one + 5, sign, 0, sign | one, 1, 2]
    for r in (0, 1):
        at = rng.integers(0, cols, size=min(cols, 24))
        x[r, at] = np.resize(np.array(plant, dtype=x.dtype), at.size)
        x[r, rng.integers(0, cols, size=cols // 3)] = x[r, 0]  # a large tie block
    x[2] = np.where(rng.random(cols) < 0.5, 0, sign | one).astype(x.dtype)
    return x
