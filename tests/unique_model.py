"""The contract of labsort_unique_device (include/labsort.h) as a numpy model: two keys are one value
when their order images are equal (tests/f32_model.py and tests/sort64_model.py have the images), the
default mode is a stable argsort of the images followed by the run edges, consecutive mode the run
edges of the input as it lies.  Arrays are uint32 or uint64 words; kind is "u32", "i32", "f32", "u64",
"i64" or "f64".  Nothing here calls the library."""
import functools

import numpy as np

import f32_model as F
import sort64_model as M

KINDS32 = ("u32", "i32", "f32")
KINDS64 = M.KINDS
KINDS = KINDS32 + KINDS64
KT = {"u32": 0, "i32": 1, "f32": 2, **M.KT}
SENTINEL32 = 0xA5A5A5A5  # what the tests pre-fill the outputs with


def word_dtype(kind):
    return np.uint64 if kind in KINDS64 else np.uint32


def image(x, kind):
    if kind in KINDS64:
        return M.ord64(x, kind)
    x = np.asarray(x, dtype=np.uint32)
    if kind == "f32":
        return F.ord_bits(x)
    return x ^ np.uint32(0x80000000) if kind == "i32" else x.copy()


def from_image(o, kind):
    if kind in KINDS64:
        return M.unord64(o, kind)
    o = np.asarray(o, dtype=np.uint32)
    if kind == "f32":
        return F.unord_bits(o)
    return o ^ np.uint32(0x80000000) if kind == "i32" else o.copy()


def expected(x, kind, consecutive=False):
    """(values, counts, first, inverse, m) of a 1-D array of words: values of the words' dtype (a NaN
    as 0x7FFF..), the other three uint32."""
    x = np.asarray(x, dtype=word_dtype(kind))
    n = x.size
    if n == 0:
        e = np.zeros(0, dtype=np.uint32)
        return x.copy(), e, e.copy(), e.copy(), 0
    u = image(x, kind)
    order = np.arange(n) if consecutive else np.argsort(u, kind="stable")
    s = u[order]
    head = np.ones(n, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    start = np.flatnonzero(head)
    m = start.size
    values = from_image(s[start], kind).astype(x.dtype)
    counts = np.diff(np.append(start, n)).astype(np.uint32)
    first = order[start].astype(np.uint32)  # (stable: the lowest position of the value, or the run's start)
    inverse = np.empty(n, dtype=np.uint32)
    inverse[order] = (np.cumsum(head) - 1).astype(np.uint32)
    return values, counts, first, inverse, m


def from_ints(v, kind):
    """Integer values as keys of the kind: the float of the value, or its two's complement word."""
    v = np.asarray(v, dtype=np.int64)
    if kind == "f32":
        return v.astype(np.float32).view(np.uint32).copy()
    if kind == "f64":
        return v.astype(np.float64).view(np.uint64).copy()
    return v.astype(np.int32).view(np.uint32).copy() if kind in KINDS32 else v.view(np.uint64).copy()


GENERATORS = ("uniform", "mod17", "mod1000", "sorted_runs")


def generate(gen, n, seed, kind):
    """uniform: full-width random words; mod17 / mod1000: few distinct values; sorted_runs: ascending
    with long runs (one value per 1 .. 3000 elements)."""
    rng = np.random.default_rng(seed)
    bits = 64 if kind in KINDS64 else 32
    if gen == "uniform":
        return rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(word_dtype(kind))
    if gen in ("mod17", "mod1000"):
        return from_ints(rng.integers(0, 1 << 40, size=n) % (17 if gen == "mod17" else 1000) - 5, kind)
    if gen == "sorted_runs":
        lens = rng.integers(1, 3001, size=n // 1000 + 2)
        low = 0 if kind in ("u32", "u64") else lens.size  # (signed kinds start below zero)
        v = np.repeat(np.arange(lens.size, dtype=np.int64) * 3 - low, lens)
        while v.size < n:
            v = np.concatenate([v, v + (v[-1] - v[0] + 1)])
        return from_ints(v[:n], kind)
    raise ValueError(gen)


def freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(gen, n, seed, kind, consecutive):
    """An input and its expected outputs, computed once and shared (read-only)."""
    x = generate(gen, n, seed, kind)
    exp = expected(x, kind, consecutive)
    freeze(x, *exp)
    return x, exp


def sizes(C):
    """The sizes at which the entry takes another path: one wave's worth, a chunk's edges, several
    chunks, and past the key/value sort's switch to its radix path."""
    return [1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5, (1 << 18) + 3]


def route_sizes(pair_tile, tile, keys_merge_max, pairs_merge_max):
    """(id, n) at one below, at and one above every size at which an inner sort of the 4-byte keys
    changes algorithm below the gathered radix's end: the key/value tile, the keys-only tile, the
    keys' and the pairs' switch from the merge sort to a radix."""
    edges = (("pair_tile", pair_tile), ("tile", tile), ("2^16", keys_merge_max), ("2^18", pairs_merge_max))
    return [(f"{name}{d:+d}" if d else name, e + d) for name, e in edges for d in (-1, 0, 1)]


SPREAD_A = {32: 0x9E3779B1, 64: 0x9E3779B97F4A7C15}  # odd: v -> v * A mod 2^bits is a bijection
INT_KINDS = ("u32", "i32", "u64", "i64")


def spread_values(V, kind):
    """The words (v * A) mod 2^bits for v = 0 .. V - 1: distinct, and different in every digit."""
    if kind not in INT_KINDS:
        raise ValueError(f"spread: an integer kind expected (float images merge NaNs), got {kind}")
    bits = 64 if kind in KINDS64 else 32
    b = np.arange(V, dtype=np.uint64) * np.uint64(SPREAD_A[bits])  # (wraps mod 2^64)
    return (b & np.uint64((1 << bits) - 1)).astype(word_dtype(kind))


def spread(n, V, kind):
    """x[i] = ((i mod V) * A) mod 2^bits: V distinct values in turn, n elements."""
    return np.resize(spread_values(V, kind), n)


def spread_expected(n, V, kind):
    """expected(spread(n, V, kind), kind) in closed form: only the min(V, n) values are sorted.  Value
    v occurs at v, v + V, ...: n // V times and once more if v < n % V, first at v."""
    assert n >= 1 and V >= 1
    m = min(V, n)
    b = spread_values(V, kind)[:m]
    order = np.argsort(image(b, kind), kind="stable")  # order[j]: the v of the j-th smallest value
    values = b[order]
    counts = (n // V + (order < n % V)).astype(np.uint32)
    first = order.astype(np.uint32)
    rank = np.empty(m, dtype=np.uint32)
    rank[order] = np.arange(m, dtype=np.uint32)
    return values, counts, first, np.resize(rank, n), m


def sweep_cases(seed, C, count=40):
    """The seeded sweep: size, key type, mode, output combination and generator drawn per case."""
    rng = np.random.default_rng(seed)
    ns = sizes(C)
    for i in range(count):
        n = ns[int(rng.integers(0, len(ns)))]
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        gen = GENERATORS[int(rng.integers(0, len(GENERATORS)))]
        yield dict(n=n, kind=kind, gen=gen, consecutive=bool(rng.integers(0, 2)), outputs=int(rng.integers(0, 8)),
                   seed=seed * 1000 + i, tag=f"{kind} n={n} {gen}")
