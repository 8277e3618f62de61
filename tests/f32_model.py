"""The float32 key contract of include/labsort.h as an independent numpy model, shared by the
test_f32_* files: the order image ord / unord, the expected outputs by numpy's stable argsort of
it, the comparison rule (NaN-ness equal everywhere, every other word bit-exact) and the input
generators.  Nothing here calls the library."""
import numpy as np

SPECIALS = {
    "+0": 0x00000000, "-0": 0x80000000, "+inf": 0x7F800000, "-inf": 0xFF800000,
    "qnan": 0x7FC00000, "-qnan1": 0xFFC00001, "snan": 0x7F800001,
    "+denorm_min": 0x00000001, "-denorm_min": 0x80000001, "+flt_max": 0x7F7FFFFF, "-flt_max": 0xFF7FFFFF,
}
PLANTED = np.array(sorted(SPECIALS.values()), dtype=np.uint32)


def is_nan(x):
    x = np.asarray(x, dtype=np.uint32)
    return (x & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def ord_bits(x):
    """ord(x): 0xFFFFFFFF for a NaN, ~x with the sign bit set, x | 0x80000000 otherwise."""
    x = np.asarray(x, dtype=np.uint32)
    o = np.where((x & np.uint32(0x80000000)) != 0, ~x, x | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(is_nan(x), np.uint32(0xFFFFFFFF), o).astype(np.uint32)


def unord_bits(o):
    o = np.asarray(o, dtype=np.uint32)
    return np.where((o & np.uint32(0x80000000)) != 0, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)


def u_of(x, largest=False):
    return ord_bits(x) ^ np.uint32(0xFFFFFFFF if largest else 0)


def assert_keys(got, want, msg=""):
    """NaN-ness equal everywhere, all other words bit-exact."""
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    gn, wn = is_nan(got), is_nan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"NaN positions: {msg}")
    np.testing.assert_array_equal(np.where(gn, np.uint32(0), got), np.where(wn, np.uint32(0), want), err_msg=f"keys: {msg}")


def topk_expected(x, k, largest):
    """x: (rows, cols) words.  The first k of each row's stable sort on u, and their positions."""
    idx = np.argsort(u_of(x, largest), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def sort_expected(x, vals=None):
    """Stable ascending sort of a 1-D array of words (and the payloads carried with it)."""
    p = np.argsort(ord_bits(x), kind="stable")
    return (x[p], None) if vals is None else (x[p], vals[p])


def segments_expected(x, off, vals=None):
    ek = x.copy()
    ev = None if vals is None else vals.copy()
    for a, b in zip(off[:-1], off[1:]):
        if b - a > 1:
            p = np.argsort(ord_bits(x[a:b]), kind="stable")
            ek[a:b] = x[a:b][p]
            if vals is not None:
                ev[a:b] = vals[a:b][p]
    return ek, ev


def random_words(shape, seed, plant=True):
    """Random 32-bit words read as floats: about 0.4 % NaN of both signs (exponent all ones) and as
    many denormals; with plant, the special values at random places (where the array has room)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    if plant and x.size >= 4 * PLANTED.size:
        flat = x.reshape(-1)
        at = rng.choice(flat.size, size=2 * PLANTED.size, replace=False)
        flat[at] = np.tile(PLANTED, 2)
    return x


def normal_words(shape, seed):
    """Standard-normal float32 values, as words (their top byte is concentrated)."""
    return np.random.default_rng(seed).standard_normal(size=shape, dtype=np.float32).view(np.uint32).copy()


def tie_words(shape, seed):
    """Heavy ties: normals rounded to 8 values, NaNs of several payloads and both zeros."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal(size=shape) * 1.5).clip(-3, 4).astype(np.float32)).view(np.uint32).copy()
    r = rng.random(size=shape)
    x[r < 0.10] = 0x80000000
    x[(r >= 0.10) & (r < 0.20)] = 0x00000000
    x[(r >= 0.20) & (r < 0.25)] = 0x7FC00000
    x[(r >= 0.25) & (r < 0.28)] = 0xFFC00001
    x[(r >= 0.28) & (r < 0.30)] = 0x7F800001
    return x
