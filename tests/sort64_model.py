"""The contract of labsort_sort64_device (include/labsort.h) as a numpy model: the order images of the
three 8-byte key types and their inverses, the expected keys and positions of a call, which of the
eight bytes of the images vary over a matrix, and generators of inputs.  Arrays are uint64 words; kind
is "u64", "i64" or "f64".  Nothing here calls the library."""
import functools

import numpy as np

KINDS = ("u64", "i64", "f64")
KT = {"u64": 8, "i64": 9, "f64": 10}
SIGN = np.uint64(1 << 63)
MAG = np.uint64((1 << 63) - 1)
INF = np.uint64(0x7FF0000000000000)
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_OUT = 0x7FFFFFFFFFFFFFFF  # how every NaN comes back


def words(x):
    return np.ascontiguousarray(x).view(np.uint64) if np.asarray(x).dtype != np.uint64 else np.asarray(x)


def is_nan(x):
    return (words(x) & MAG) > INF


def ord64(x, kind):
    x = words(x)
    if kind == "u64":
        return x.copy()
    if kind == "i64":
        return x ^ SIGN
    o = np.where((x & SIGN) != 0, ~x, x | SIGN)
    return np.where(is_nan(x), ALL1, o)


def unord64(o, kind):
    o = np.asarray(o, dtype=np.uint64)
    if kind == "u64":
        return o.copy()
    if kind == "i64":
        return o ^ SIGN
    return np.where((o >> np.uint64(63)) != 0, o & MAG, ~o)


def u_of(x, kind, descending=False):
    return ord64(x, kind) ^ (ALL1 if descending else np.uint64(0))


def expected(x, descending, kind):
    """x: (rows, cols) words.  Each row's stable sort on u with the keys taken through the inverse
    image (every NaN comes back as NAN_OUT), and the positions."""
    u = u_of(x, kind, descending)
    idx = np.argsort(u, axis=1, kind="stable")
    keys = unord64(np.take_along_axis(ord64(x, kind), idx, axis=1), kind)
    return keys, idx.astype(np.uint32)


def active_bytes(x, kind, descending=False):
    """The set of bytes p in which the images of the matrix's keys differ, as a bitmask."""
    u = u_of(x, kind, descending).reshape(-1)
    vary = int(np.bitwise_or.reduce(u)) & int(np.bitwise_or.reduce(~u))
    return sum(1 << p for p in range(8) if (vary >> (8 * p)) & 0xFF)


def byte_set(mask):
    return [p for p in range(8) if (mask >> p) & 1]


def rows_with_bytes(shape, mask, seed, kind="u64"):
    """(rows, cols >= 2) keys whose images differ in exactly the bytes of `mask`, in every row: the
    other bytes are one random constant, a byte of the set is random per key and takes a value and its
    complement in the row's first two keys.  Byte 7 stays in [0x10, 0xEF], so that every word is the
    image of a float64 that is no NaN."""
    rows, cols = shape
    assert cols >= 2
    rng = np.random.default_rng(seed)
    img = np.zeros(shape, dtype=np.uint64)
    for p in range(8):
        lo, hi = (0x10, 0xF0) if p == 7 else (0, 256)
        if (mask >> p) & 1:
            b = rng.integers(lo, hi, size=shape, dtype=np.uint64)
            at = rng.integers(0, cols - 1, size=rows)  # two neighbours somewhere in the row
            r = np.arange(rows)
            b[r, at + 1] = b[r, at] ^ np.uint64(0xFF)
        else:
            b = np.full(shape, rng.integers(lo, hi), dtype=np.uint64)
        img |= b << np.uint64(8 * p)
    return unord64(img, kind)


F64_SPECIALS = np.array([
    0x0000000000000000, 0x8000000000000000,  # +0.0, -0.0
    0x7FF0000000000000, 0xFFF0000000000000,  # +inf, -inf
    0x7FF8000000000000, 0xFFF8000000000001,  # quiet NaNs of both signs
    0x7FF0000000000001, 0xFFF4000000000000,  # signalling NaNs of both signs
    0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
    0x0000000000000001, 0x8000000000000001,  # the smallest denormals
    0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,  # the largest denormals
    0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,  # the smallest normal, +-max
    0x3FF0000000000000, 0xBFF0000000000000], dtype=np.uint64)
INT_SPECIALS = np.array([
    0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0, 1,  # i64: min, max, -1, 0, 1
    0x8000000000000001, 0x7FFFFFFFFFFFFFFE, 0x00000000FFFFFFFF, 0x0000000100000000, 0xFFFFFFFF00000000], dtype=np.uint64)


def specials(kind):
    return F64_SPECIALS if kind == "f64" else INT_SPECIALS


def _from_ints(v, kind):
    """int64 values as keys of the kind: the float64 of the value, or its two's complement word."""
    v = np.asarray(v, dtype=np.int64)
    return v.astype(np.float64).view(np.uint64) if kind == "f64" else v.view(np.uint64).copy()


GENERATORS = ("random", "ties", "narrow", "sorted", "reversed", "mixed_sign_small", "nan_heavy")


def generate(gen, shape, seed, kind):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    if gen == "random":
        x = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    elif gen == "ties":
        x = _from_ints(rng.integers(0, 1 << 40, size=shape) % 3, kind)
    elif gen == "narrow":
        x = _from_ints(rng.integers(0, 1 << 20, size=shape), kind)
    elif gen in ("sorted", "reversed"):
        v = (np.arange(n, dtype=np.int64) * 7 - 3 * (n // 2)).reshape(shape)  # across zero
        x = _from_ints(v if gen == "sorted" else v[:, ::-1], kind)
    elif gen == "mixed_sign_small":
        x = _from_ints(rng.integers(-1000, 1001, size=shape), kind)
    elif gen == "nan_heavy":
        x = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
        s = specials(kind)
        heavy = s[is_nan(s)] if kind == "f64" else s[:3]
        at = rng.random(shape) < 0.5
        x[at] = heavy[rng.integers(0, heavy.size, size=int(at.sum()))]
    else:
        raise ValueError(gen)
    return np.ascontiguousarray(x, dtype=np.uint64)


def planted(shape, seed, kind):
    """Random words with the kind's special values scattered through every row."""
    x = generate("random", shape, seed, kind)
    rng = np.random.default_rng(seed + 1)
    s = specials(kind)
    for r in range(shape[0]):
        at = rng.integers(0, shape[1], size=min(shape[1], 4 * s.size))
        x[r, at] = np.resize(s, at.size)
    return x


def make_case(kind, rows, cols, seed=0x6401):
    """An input and its expected outputs in both directions (read-only): random words with planted
    specials, every third row heavy ties."""
    x = planted((rows, cols), seed + rows + cols, kind)
    x[::3] = generate("ties", (rows, cols), seed + cols, kind)[::3]
    exp = {d: expected(x, d, kind) for d in (False, True)}
    x.setflags(write=False)
    for ek, ei in exp.values():
        ek.setflags(write=False)
        ei.setflags(write=False)
    return x, exp


@functools.lru_cache(maxsize=None)
def case(kind, rows, cols, seed=0x6401):
    """make_case, computed once and shared among the tests that use the shape."""
    return make_case(kind, rows, cols, seed)


def sweep_cases(seed, C, count=40):
    """The seeded sweep: rows in 1 .. 5, cols up to 3 C (half of them at a chunk edge +-1), key type,
    direction, positions and generator drawn per case."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        rows = int(rng.integers(1, 6))
        if rng.random() < 0.5:
            cols = int(rng.integers(1, 4)) * C + int(rng.integers(-1, 2))
        else:
            cols = int(rng.integers(1, 3 * C + 1))
        cols = max(1, min(cols, 3 * C))
        kind = KINDS[int(rng.integers(0, 3))]
        gen = GENERATORS[int(rng.integers(0, len(GENERATORS)))]
        yield dict(rows=rows, cols=cols, kind=kind, gen=gen, descending=bool(rng.integers(0, 2)),
                   with_idx=bool(rng.integers(0, 2)), x=generate(gen, (rows, cols), seed * 1000 + i, kind),
                   tag=f"{kind} {rows}x{cols} {gen}")
