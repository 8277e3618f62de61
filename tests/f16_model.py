"""The 16-bit float key contract of include/labsort.h (LABSORT_KEY_BF16, LABSORT_KEY_F16) as an
independent numpy model, shared by the test_f16_* files: the order image ord16 / unord16 per type,
the expected top-k outputs by numpy's stable argsort of it, the comparison rule (NaN-ness equal
everywhere, every other element bit-exact) and the input generators.  Arrays are uint16 words;
kind is "bf16" or "f16".  Nothing here calls the library."""
import numpy as np

INF = {"bf16": 0x7F80, "f16": 0x7C00}  # the word of +inf: above it (sign cleared) a word is a NaN
KINDS = ("bf16", "f16")


def specials(kind):
    t = INF[kind]
    return {
        "+0": 0x0000, "-0": 0x8000, "+inf": t, "-inf": 0x8000 | t,
        "qnan": 0x7FC0 if kind == "bf16" else 0x7E00, "-qnan1": 0xFFC1 if kind == "bf16" else 0xFE01,
        "snan": t | 1, "-snan": 0x8000 | t | 2,  # signalling: the quiet bit clear, a payload bit set
        "+denorm_min": 0x0001, "-denorm_min": 0x8001, "+max": t - 1, "-max": 0x8000 | (t - 1),
    }


def planted(kind):
    return np.array(sorted(specials(kind).values()), dtype=np.uint16)


def is_nan16(x, kind):
    x = np.asarray(x, dtype=np.uint16)
    return (x & np.uint16(0x7FFF)) > np.uint16(INF[kind])


def ord16(x, kind):
    """0xFFFF for a NaN, ~x with the sign bit set, x | 0x8000 otherwise."""
    x = np.asarray(x, dtype=np.uint16)
    o = np.where((x & np.uint16(0x8000)) != 0, ~x, x | np.uint16(0x8000)).astype(np.uint16)
    return np.where(is_nan16(x, kind), np.uint16(0xFFFF), o).astype(np.uint16)


def unord16(o):
    o = np.asarray(o, dtype=np.uint16)
    return np.where((o & np.uint16(0x8000)) != 0, o & np.uint16(0x7FFF), ~o).astype(np.uint16)


def u_of(x, kind, largest=False):
    return ord16(x, kind) ^ np.uint16(0xFFFF if largest else 0)


def assert_keys(got, want, kind, msg=""):
    """NaN-ness equal everywhere, all other elements bit-exact."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    gn, wn = is_nan16(got, kind), is_nan16(want, kind)
    np.testing.assert_array_equal(gn, wn, err_msg=f"NaN positions: {msg}")
    np.testing.assert_array_equal(np.where(gn, np.uint16(0), got), np.where(wn, np.uint16(0), want), err_msg=f"keys: {msg}")


def topk_expected(x, k, largest, kind):
    """x: (rows, cols) words.  The first k of each row's stable sort on u, and their positions."""
    idx = np.argsort(u_of(x, kind, largest), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def as_float32(x, kind):
    """The values of the words as float32 (exact for both formats)."""
    x = np.asarray(x, dtype=np.uint16)
    if kind == "bf16":
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return x.view(np.float16).astype(np.float32)


def random_words(shape, seed, kind, plant=True):
    """Random 16-bit words read as floats (bf16: 0.4 % NaN, f16: 3 %, of both signs); with plant, the
    special values at random places (where the array has room)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 16, size=shape, dtype=np.uint32).astype(np.uint16)
    p = planted(kind)
    if plant and x.size >= 4 * p.size:
        flat = x.reshape(-1)
        at = rng.choice(flat.size, size=2 * p.size, replace=False)
        flat[at] = np.tile(p, 2)
    return x


def normal_words(shape, seed, kind):
    """Standard normals rounded to the type: float16 by astype, bfloat16 by rounding the float32
    word to its top 16 bits (to nearest, ties to even)."""
    f = np.random.default_rng(seed).standard_normal(size=shape, dtype=np.float32)
    if kind == "f16":
        return f.astype(np.float16).view(np.uint16).copy()
    w = f.view(np.uint32)
    w = w + np.uint32(0x7FFF) + ((w >> np.uint32(16)) & np.uint32(1))
    return (w >> np.uint32(16)).astype(np.uint16)


def tie_words(shape, seed, kind):
    """Heavy ties: normals rounded to 8 integers (exact in both formats), NaNs of several payloads
    and both zeros."""
    rng = np.random.default_rng(seed)
    f = np.round(rng.standard_normal(size=shape) * 1.5).clip(-3, 4).astype(np.float32)
    x = f.astype(np.float16).view(np.uint16).copy() if kind == "f16" else (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    s = specials(kind)
    r = rng.random(size=shape)
    x[r < 0.10] = s["-0"]
    x[(r >= 0.10) & (r < 0.20)] = s["+0"]
    x[(r >= 0.20) & (r < 0.25)] = s["qnan"]
    x[(r >= 0.25) & (r < 0.28)] = s["-qnan1"]
    x[(r >= 0.28) & (r < 0.30)] = s["snan"]
    return x


def to_torch(x, kind, torch):
    """A CPU tensor of the type over a copy of the words."""
    t = torch.from_numpy(np.ascontiguousarray(x).view(np.int16).copy())
    return t.view(torch.bfloat16 if kind == "bf16" else torch.float16)
