"""The dense row sort's contract (labsort_sort_rows_device, include/labsort.h) as a numpy model over
the existing ones: f16_model / f32_model's topk_expected with k = cols for the float key types, the
stable argsort of x ^ flip for the integer ones.  Arrays are words (uint16 for "bf16" / "f16",
uint32 otherwise); kind is a key of ls.KEY.  Nothing here calls the library."""
import functools

import numpy as np

import f16_model as M
import f32_model as F

KINDS = ("u32", "i32", "f32", "bf16", "f16")
KT = {"u32": 0, "i32": 1, "f32": 2, "bf16": 3, "f16": 4}


def is16(kind):
    return kind in M.KINDS


def wdtype(kind):
    return np.uint16 if is16(kind) else np.uint32


def u_of(x, kind, descending=False):
    if is16(kind):
        return M.u_of(x, kind, descending)
    if kind == "f32":
        return F.u_of(x, descending)
    flip = (0x80000000 if kind == "i32" else 0) ^ (0xFFFFFFFF if descending else 0)
    return np.asarray(x, dtype=np.uint32) ^ np.uint32(flip)


def expected(x, descending, kind):
    """x: (rows, cols) words.  Each row's stable sort on u, and the positions."""
    cols = x.shape[1]
    if is16(kind):
        return M.topk_expected(x, cols, descending, kind)
    if kind == "f32":
        return F.topk_expected(x, cols, descending)
    idx = np.argsort(u_of(x, kind, descending), axis=1, kind="stable")
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def assert_keys(got, want, kind, msg=""):
    """Bit-exact, except that for the float types a NaN only has to be a NaN."""
    if is16(kind):
        M.assert_keys(got, want, kind, msg)
    elif kind == "f32":
        F.assert_keys(got, want, msg)
    else:
        np.testing.assert_array_equal(np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32), err_msg=f"keys: {msg}")


def nan_word(kind):
    """A key that is last ascending and whose image equals the padding's: a NaN, or the largest integer."""
    if is16(kind):
        return M.specials(kind)["-qnan1"]
    return {"f32": 0xFFC00001, "u32": 0xFFFFFFFF, "i32": 0x7FFFFFFF}[kind]


INT_TIES = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF, 0x00010000, 0xFFFF0000], dtype=np.uint32)


def random_words(shape, seed, kind):
    if is16(kind):
        return M.random_words(shape, seed, kind)
    if kind == "f32":
        return F.random_words(shape, seed)
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def tie_words(shape, seed, kind):
    """Heavy ties; the float kinds with NaNs of several payloads and both zeros."""
    if is16(kind):
        return M.tie_words(shape, seed, kind)
    if kind == "f32":
        return F.tie_words(shape, seed)
    return INT_TIES[np.random.default_rng(seed).integers(0, INT_TIES.size, size=shape)]


def planted_words(shape, seed, kind):
    """Random words with special values planted: both zeros, infinities, NaNs of both signs, quiet and
    signalling (floats); the extremes of both integer orders."""
    x = random_words(shape, seed, kind)
    rng = np.random.default_rng(seed + 1)
    p = M.planted(kind) if is16(kind) else F.PLANTED if kind == "f32" else INT_TIES
    flat = x.reshape(-1)
    at = rng.integers(0, flat.size, size=min(flat.size, 4 * p.size))
    flat[at] = np.resize(p, at.size)
    return x


def make_case(kind, rows, cols, gen="mixed", seed=0x5041):
    """An input and its expected outputs in both directions (read-only).
    mixed: random words with planted specials, every third row heavy ties."""
    if gen == "mixed":
        x = planted_words((rows, cols), seed + rows + cols, kind)
        x[::3] = tie_words((rows, cols), seed + cols, kind)[::3]
    elif gen == "random":
        x = random_words((rows, cols), seed + rows + cols, kind)
    else:
        x = tie_words((rows, cols), seed + rows + cols, kind)
    x = np.ascontiguousarray(x, dtype=wdtype(kind))
    exp = {d: expected(x, d, kind) for d in (False, True)}
    x.setflags(write=False)
    for ek, ei in exp.values():
        ek.setflags(write=False)
        ei.setflags(write=False)
    return x, exp


@functools.lru_cache(maxsize=None)
def case(kind, rows, cols, gen="mixed", seed=0x5041):
    """make_case, computed once and shared among the tests that use the shape."""
    return make_case(kind, rows, cols, gen, seed)
