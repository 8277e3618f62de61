"""The contract of labsort_searchsorted_device (include/labsort.h) as a numpy model: the rank of a
value in a sequence is the number of the sequence's elements whose order image is below (right: not
above) the value's, which on an ascending sequence is np.searchsorted on the images.  The images are
those of tests/f32_model.py, tests/f16_model.py and tests/sort64_model.py.  Arrays are uint16, uint32
or uint64 words; kind is one of KINDS.  Nothing here calls the library."""
import functools

import numpy as np

import f16_model as M16
import f32_model as F
import sort64_model as M64

KINDS16 = M16.KINDS
KINDS32 = ("u32", "i32", "f32")
KINDS64 = M64.KINDS
KINDS = KINDS32 + KINDS16 + KINDS64
FLOATS = ("f32", "bf16", "f16", "f64")
KT = {"u32": 0, "i32": 1, "f32": 2, "bf16": 3, "f16": 4, **M64.KT}
SENTINEL = 0xA5A5A5A5  # what the tests pre-fill the output and its canaries with
SAMPLES = 4096         # sample images per sequence on the long path (labsort.h)


def word_dtype(kind):
    return np.uint16 if kind in KINDS16 else np.uint64 if kind in KINDS64 else np.uint32


def esz(kind):
    return np.dtype(word_dtype(kind)).itemsize


def image(x, kind):
    if kind in KINDS64:
        return M64.ord64(np.asarray(x, dtype=np.uint64), kind)
    if kind in KINDS16:
        return M16.ord16(np.asarray(x, dtype=np.uint16), kind).astype(np.uint16)
    x = np.asarray(x, dtype=np.uint32)
    if kind == "f32":
        return F.ord_bits(x)
    return x ^ np.uint32(0x80000000) if kind == "i32" else x.copy()


def from_image(o, kind):
    """A word with the image o (the NaN image gives 0x7FFF..)."""
    if kind in KINDS64:
        return M64.unord64(np.asarray(o, dtype=np.uint64), kind).astype(np.uint64)
    if kind in KINDS16:
        return M16.unord16(np.asarray(o, dtype=np.uint16)).astype(np.uint16)
    o = np.asarray(o, dtype=np.uint32)
    if kind == "f32":
        return F.unord_bits(o).astype(np.uint32)
    return o ^ np.uint32(0x80000000) if kind == "i32" else o.copy()


def ascending(x, kind):
    """The words of x (the last axis) in ascending image order, equal images in input order."""
    x = np.asarray(x, dtype=word_dtype(kind))
    return np.take_along_axis(x, np.argsort(image(x, kind), axis=-1, kind="stable"), axis=-1)


def expected(seq, values, right, kind, sorter=None):
    """The ranks, uint32 of values' shape.  seq: 1-D (every value is searched in it) or 2-D (row r of the
    2-D values in row r); sorter: None or positions of seq's shape that put each row in order."""
    seq, values = np.asarray(seq, dtype=word_dtype(kind)), np.asarray(values, dtype=word_dtype(kind))
    side = "right" if right else "left"
    u, v = image(seq, kind), image(values, kind)
    if sorter is not None:
        u = np.take_along_axis(u, np.asarray(sorter).astype(np.int64), axis=-1)
    if seq.ndim == 1:
        return np.searchsorted(u, v.ravel(), side=side).astype(np.uint32).reshape(values.shape)
    assert seq.ndim == 2 and values.ndim == 2 and seq.shape[0] == values.shape[0]
    out = np.empty(values.shape, dtype=np.uint32)
    for r in range(seq.shape[0]):
        out[r] = np.searchsorted(u[r], v[r], side=side)
    return out


def loop_ranks(seq, values, right, kind):
    """The definition, one comparison at a time (for the model's own test; 1-D, small)."""
    u, v = [int(t) for t in image(seq, kind)], [int(t) for t in image(values, kind)]
    return np.array([sum(1 for e in u if (e <= t if right else e < t)) for t in v], dtype=np.uint32)


# ---- words that can go wrong
def float_specials(kind):
    """NaNs of several payloads and both signs, both zeros, both infinities, the finite extremes."""
    if kind == "f32":
        return np.array(sorted(F.SPECIALS.values()) + [0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF],
                        dtype=np.uint32)
    if kind in KINDS16:
        return np.array(sorted(M16.specials(kind).values()) + [0x7FFF, 0xFFFF], dtype=np.uint16)
    assert kind == "f64"
    return np.concatenate([M64.F64_SPECIALS, np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001,
                                                       0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0], dtype=np.uint64)])


def probes(seq, kind):
    """Values around a sequence: every element, the words one image below and above each, the smallest
    and the largest image, and for the float kinds the specials."""
    dt = word_dtype(kind)
    u = image(np.asarray(seq, dtype=dt).ravel(), kind)
    top = dt(np.iinfo(dt).max)
    one = dt(1)
    below = np.where(u > 0, u - one, u)
    above = np.where(u < top, u + one, u)
    parts = [np.asarray(seq, dtype=dt).ravel(), from_image(below, kind), from_image(above, kind),
             from_image(np.array([0, 1, top - one, top], dtype=dt), kind)]
    if kind in FLOATS:
        parts.append(float_specials(kind))
    return np.concatenate(parts).astype(dt)


def random_words(n, seed, kind):
    rng = np.random.default_rng(seed)
    bits = 8 * esz(kind)
    return rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(word_dtype(kind))


@functools.lru_cache(maxsize=1024)
def sequence(gen, cols, seed, kind):
    """An ascending sequence of cols words (read-only, shared).  random: full-width words (for the
    float kinds with the specials planted); equal: one key; two: two distinct keys; few: about cols / 600 distinct keys in
    runs of every length up to about 1200, so that with cols >= 2^15 many runs cover several strides
    of the long path's table; runs:<len>: runs of exactly len elements (the last one shorter)."""
    rng = np.random.default_rng([seed, cols, KT[kind]])
    dt = word_dtype(kind)
    if cols == 0:
        return freeze(np.zeros(0, dtype=dt))[0]
    x = random_words(cols, int(rng.integers(0, 1 << 31)), kind)
    if gen == "random":
        if kind in FLOATS:
            s = float_specials(kind)
            at = rng.integers(0, cols, size=min(cols, 2 * s.size))
            x[at] = s[rng.integers(0, s.size, size=at.size)]
    elif gen == "equal":
        x[:] = x[0]
    elif gen == "two":
        x = np.where(rng.random(cols) < 0.5, x[0], x[-1] if image(x[-1:], kind)[0] != image(x[:1], kind)[0] else ~x[0])
    elif gen == "few":
        k = min(cols, max(2, cols // 600))
        x = x[:k][rng.integers(0, k, size=cols)]
    elif gen.startswith("runs:"):
        ln = int(gen.split(":")[1])
        k = (cols + ln - 1) // ln
        x = np.repeat(from_image(np.sort(np.unique(image(x[:max(k, 1)], kind))), kind), ln)
        while x.size < cols:  # (the draws held equal images)
            x = np.concatenate([x, x[-1:]])
        x = x[:cols]
    else:
        raise ValueError(gen)
    return freeze(ascending(x.astype(dt), kind))[0]


def half_words(cols, seed, which):
    """uint64 words that differ in one half only (which: 'lo' or 'hi'), above 2^63 for 'lo'."""
    rng = np.random.default_rng([seed, cols])
    r = rng.integers(0, 1 << 32, size=cols, dtype=np.uint64)
    return (np.uint64(0xFFFFFFFE) << np.uint64(32)) | r if which == "lo" else (r << np.uint64(32)) | np.uint64(0x89ABCDEF)


def freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=512)
def shared_case(gen, cols, nv, seed, kind):
    """(sequence, values, ranks left, ranks right) with one sequence, computed once and shared
    (read-only).  The values are nv of the sequence's probes: all of them, repeated, when there are
    fewer, a random choice otherwise."""
    seq = sequence(gen, cols, seed, kind)
    p = probes(seq, kind) if cols else random_words(64, seed, kind)
    rng = np.random.default_rng([seed, nv, 7])
    vals = np.resize(p, nv) if p.size <= nv else p[rng.choice(p.size, size=nv, replace=False)]
    return freeze(seq, vals, expected(seq, vals, False, kind), expected(seq, vals, True, kind))


@functools.lru_cache(maxsize=16)
def row_case(gen, rows, cols, nv, seed, kind):
    """The same with a sequence per row: (rows x cols, rows x nv, left, right)."""
    seq = np.stack([sequence(gen, cols, seed + r, kind) for r in range(rows)]) if cols else \
        np.zeros((rows, 0), dtype=word_dtype(kind))
    vals = np.stack([shared_case(gen, cols, nv, seed + r, kind)[1] for r in range(rows)])
    return freeze(seq, vals, expected(seq, vals, False, kind), expected(seq, vals, True, kind))


def cols_sizes(L):
    """The sequence lengths at which the entry takes another path or another stride: L the longest
    sequence of the LDS path."""
    k0 = L // SAMPLES
    past = [SAMPLES * k + d for k in (k0 + 1, k0 + 2) for d in (-1, 0, 1)]
    return [0, 1, 2, 3, 63, 64, 65, L - 1, L, L + 1] + past + [3 * (1 << 20) + 5]


def nv_sizes(V):
    return [1, 7, 8, 9, V - 1, V, V + 1, 3 * V + 5]


def sweep_words(kind, n, rng):
    """n words from a generator of tests/sort_sweep_model.py (sort64_model.py's for the 8-byte kinds),
    drawn with rng."""
    import sort_sweep_model as S
    if kind in KINDS64:
        gen = M64.GENERATORS[int(rng.integers(0, len(M64.GENERATORS)))]
        return M64.generate(gen, (1, n), int(rng.integers(0, 1 << 31)), kind)[0]
    return np.asarray(S.sweep_row(S.pick_gen(rng, kind), n, kind, False, rng), dtype=word_dtype(kind))


def sweep_case(c):
    """(seq, values, sorter or None, expected) of a case of sweep_cases: rows of sweep_words put in
    order (or left as drawn, with the sorter that orders them); values from the rows and fresh draws."""
    rng = np.random.default_rng(c["seed"])
    kind, rows, cols, nv = c["kind"], c["rows"], c["cols"], c["nv"]
    raw = np.stack([sweep_words(kind, cols, rng) for _ in range(rows)])
    order = np.argsort(image(raw, kind), axis=-1, kind="stable")
    seq, sorter = (raw, order.astype(np.uint32)) if c["sorter"] else (np.take_along_axis(raw, order, axis=-1), None)
    vals = np.stack([np.where(rng.random(nv) < 0.5, np.resize(probes(raw[r], kind), nv)[rng.permutation(nv)],
                              sweep_words(kind, nv, rng)) for r in range(rows)]).astype(word_dtype(kind))
    if not c["per_row"]:
        seq, sorter = seq[0], None if sorter is None else sorter[0]
    return seq, vals, sorter, expected(seq, vals, c["right"], kind, sorter)


def sweep_cases(seed, row_keys, V, count=40):
    """The seeded sweep: key type, path, form, side and sorter drawn per case.  row_keys: kind -> L."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        L = row_keys[kind]
        lng = bool(rng.integers(0, 2))
        cols = int(rng.integers(L + 1, L + 3 * SAMPLES)) if lng else int(rng.integers(1, min(L, 3000) + 1))
        rows = 1 if rng.integers(0, 2) else int(rng.integers(2, 6))
        yield dict(kind=kind, cols=cols, rows=rows, per_row=rows > 1 or bool(rng.integers(0, 2)),
                   nv=int(rng.integers(1, 2 * V)), right=bool(rng.integers(0, 2)), sorter=bool(rng.integers(0, 2)),
                   seed=seed * 1000 + i, tag=f"{kind} cols={cols} rows={rows} {'long' if lng else 'lds'}")
