"""The numpy model of the 64-bit sort (tests/sort64_model.py) against numpy's own sorts and against
itself: the images order floats and integers as np.sort does, the inverse undoes them, the generator
of rows with a chosen set of varying bytes makes exactly that set, and the sweep is deterministic."""
import numpy as np
import pytest

import sort64_model as M

KINDS = pytest.mark.parametrize("kind", M.KINDS)
NPDT = {"u64": np.uint64, "i64": np.int64, "f64": np.float64}


@KINDS
def test_images_order_as_numpy_sorts(kind):
    """NaN-free data: sorting by the image gives np.sort of the values themselves, in both directions."""
    rng = np.random.default_rng(0x6410)
    if kind == "f64":
        v = np.concatenate([rng.standard_normal(4000), [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.0, 1.0]])
    else:
        v = rng.integers(0, 1 << 64, size=4000, dtype=np.uint64).view(NPDT[kind])
        v = np.concatenate([v, np.array([0, 1, -1 if kind == "i64" else 2, 1], dtype=NPDT[kind])])
    x = M.words(v.astype(NPDT[kind])).reshape(1, -1)
    for desc in (False, True):
        keys, idx = M.expected(x, desc, kind)
        got = keys.view(NPDT[kind])[0]
        want = np.sort(v)[::-1] if desc else np.sort(v)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(x[0][idx[0]], keys[0])  # bit-exact without NaNs
    # -0.0 sorts directly below +0.0
    if kind == "f64":
        z = M.ord64(np.array([0x8000000000000000, 0], dtype=np.uint64), kind)
        assert int(z[0]) + 1 == int(z[1]) == 1 << 63


@KINDS
def test_inverse_and_nans(kind):
    x = np.concatenate([M.specials(kind), np.random.default_rng(0x6411).integers(0, 1 << 64, size=1000, dtype=np.uint64)])
    o = M.ord64(x, kind)
    back = M.unord64(o, kind)
    nan = M.is_nan(x) if kind == "f64" else np.zeros(x.shape, dtype=bool)
    np.testing.assert_array_equal(back[~nan], x[~nan])
    if kind == "f64":
        assert nan.sum() >= 6
        assert np.all(o[nan] == M.ALL1) and np.all(back[nan] == np.uint64(M.NAN_OUT))
        assert o[~nan].max() < M.ALL1
        assert M.is_nan(np.uint64(M.NAN_OUT))


def test_stable_ties_and_positions():
    x = np.array([[5, 3, 5, 3, 5]], dtype=np.uint64)
    k, i = M.expected(x, False, "u64")
    assert k.tolist() == [[3, 3, 5, 5, 5]] and i.tolist() == [[1, 3, 0, 2, 4]]
    k, i = M.expected(x, True, "u64")
    assert k.tolist() == [[5, 5, 5, 3, 3]] and i.tolist() == [[0, 2, 4, 1, 3]]
    nan = np.array([[0x7FF8000000000000, 0x3FF0000000000000, 0xFFF8000000000001]], dtype=np.uint64)
    k, i = M.expected(nan, False, "f64")
    assert k.tolist() == [[0x3FF0000000000000, M.NAN_OUT, M.NAN_OUT]] and i.tolist() == [[1, 0, 2]]


@KINDS
def test_generator_makes_exactly_the_byte_set(kind):
    """All 256 sets: the generated matrix's images vary in exactly the set, in every row and in both
    directions; float64 words are never NaNs."""
    for mask in range(256):
        x = M.rows_with_bytes((3, 50), mask, 0x6420 + mask, kind)
        assert x.dtype == np.uint64 and x.shape == (3, 50)
        assert M.active_bytes(x, kind) == mask, (kind, mask)
        assert M.active_bytes(x, kind, descending=True) == mask
        for r in range(3):
            assert M.active_bytes(x[r:r + 1], kind) == mask
        if kind == "f64":
            assert not M.is_nan(x).any()
    assert M.byte_set(0b10001001) == [0, 3, 7]


def test_active_bytes_by_hand():
    assert M.active_bytes(np.array([[7, 7, 7]], dtype=np.uint64), "u64") == 0
    assert M.active_bytes(np.array([[0x0100, 0x0201]], dtype=np.uint64), "u64") == 0b11
    assert M.active_bytes(np.array([[0, 1 << 63]], dtype=np.uint64), "i64") == 0x80
    # mixed-sign small integers keep all eight bytes active
    x = M.generate("mixed_sign_small", (1, 100), 1, "i64")
    assert M.active_bytes(x, "i64") == 0xFF
    assert M.active_bytes(M.generate("narrow", (1, 5000), 1, "i64"), "i64") == 0b111


def test_generators_and_sweep():
    for kind in M.KINDS:
        for gen in M.GENERATORS:
            a, b = M.generate(gen, (2, 300), 5, kind), M.generate(gen, (2, 300), 5, kind)
            np.testing.assert_array_equal(a, b)
            assert a.dtype == np.uint64 and a.shape == (2, 300)
        assert M.is_nan(M.generate("nan_heavy", (1, 1000), 3, "f64")).sum() > 300
    cases = list(M.sweep_cases(0x64, 8192))
    assert len(cases) == 40
    assert all(1 <= c["rows"] <= 5 and 1 <= c["cols"] <= 3 * 8192 for c in cases)
    assert {c["kind"] for c in cases} == set(M.KINDS) and {c["gen"] for c in cases} == set(M.GENERATORS)
    assert {c["descending"] for c in cases} == {False, True} and {c["with_idx"] for c in cases} == {False, True}
    assert any(c["cols"] <= 8192 for c in cases) and any(c["cols"] > 8192 for c in cases)
