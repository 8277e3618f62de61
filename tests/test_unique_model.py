"""CPU tests of tests/unique_model.py, the numpy statement of labsort_unique_device's contract, against
other implementations: np.unique for the integer kinds, a plain Python loop for consecutive mode, and
the float rule (every NaN one value, -0.0 and +0.0 two) on planted inputs.  The library's own host
image functions tie the model's images to the ones the kernels compile."""
import numpy as np
import pytest

import unique_model as U

INT_KINDS = {"i32": np.int32, "u32": np.uint32, "i64": np.int64, "u64": np.uint64}


def test_library_has_the_entry(ls):
    """The model describes an entry of the library: its key-type codes are the library's."""
    assert callable(ls.unique_device) and callable(ls.unique)
    assert U.KT == {k: ls.KEY[k] for k in U.KINDS}


@pytest.mark.parametrize("kind", sorted(INT_KINDS))
@pytest.mark.parametrize("gen", U.GENERATORS)
def test_against_numpy_unique(ls, kind, gen):
    assert ls.unique_chunk_keys() > 0
    for n in (1, 2, 100, 5000):
        x = U.generate(gen, n, 0x5151 + n, kind)
        values, counts, first, inverse, m = U.expected(x, kind)
        ev, ei, einv, ec = np.unique(x.view(INT_KINDS[kind]), return_index=True, return_inverse=True, return_counts=True)
        assert m == ev.size
        np.testing.assert_array_equal(values.view(INT_KINDS[kind]), ev)
        np.testing.assert_array_equal(first, ei)
        np.testing.assert_array_equal(inverse, einv.reshape(-1))
        np.testing.assert_array_equal(counts, ec)
        assert values.dtype == U.word_dtype(kind) and counts.dtype == first.dtype == inverse.dtype == np.uint32


def runs_by_loop(img):
    values, counts, first, inverse = [], [], [], []
    for i, v in enumerate(img):
        if i == 0 or v != img[i - 1]:
            values.append(v)
            counts.append(0)
            first.append(i)
        counts[-1] += 1
        inverse.append(len(values) - 1)
    return values, counts, first, inverse


@pytest.mark.parametrize("kind", U.KINDS)
def test_consecutive_against_a_loop(ls, kind):
    assert ls.UNIQUE_CONSECUTIVE == 1
    base = np.array([3, 3, 1, 3, 3, 3, 1, 1], dtype=np.int64)
    inputs = [U.from_ints(np.tile(base, 40), kind), U.generate("mod17", 700, 7, kind), U.generate("sorted_runs", 4000, 8, kind),
              U.generate("uniform", 300, 9, kind), U.from_ints([5], kind)]
    for x in inputs:
        values, counts, first, inverse, m = U.expected(x, kind, consecutive=True)
        lv, lc, lf, li = runs_by_loop([int(v) for v in U.image(x, kind)])
        assert m == len(lv)
        np.testing.assert_array_equal(U.image(values, kind), np.array(lv, dtype=x.dtype))
        np.testing.assert_array_equal(counts, lc)
        np.testing.assert_array_equal(first, lf)
        np.testing.assert_array_equal(inverse, li)
    v, c, f, i, m = U.expected(U.from_ints(np.tile(base, 2), kind), kind, consecutive=True)
    assert m == 8 and list(c) == [2, 1, 3, 2, 2, 1, 3, 2]  # equal keys in separate runs stay separate


@pytest.mark.parametrize("kind", ("f32", "f64"))
def test_float_equality(ls, kind):
    """NaNs of three payloads and both signs are one entry, written as 0x7FFF..; the two zeros are two
    entries, -0.0 first; -inf is the smallest."""
    if kind == "f32":
        nans = [0x7FC00000, 0xFFC00001, 0x7F800001, 0xFF812345]
        mz, pz, ninf, one, canon = 0x80000000, 0, 0xFF800000, 0x3F800000, 0x7FFFFFFF
    else:
        nans = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF4000000012345]
        mz, pz, ninf, one, canon = 1 << 63, 0, 0xFFF0000000000000, 0x3FF0000000000000, 0x7FFFFFFFFFFFFFFF
    x = np.array([one, nans[0], pz, mz, nans[1], ninf, pz, nans[2], mz, one, nans[3], mz], dtype=U.word_dtype(kind))
    values, counts, first, inverse, m = U.expected(x, kind)
    assert [int(v) for v in values] == [ninf, mz, pz, one, canon] and m == 5
    assert list(counts) == [1, 3, 2, 2, 4] and list(first) == [5, 3, 2, 0, 1]
    assert list(inverse) == [3, 4, 2, 1, 4, 0, 2, 4, 1, 3, 4, 1]
    for w in x:  # the model's image is the library's
        f = ls.lib.labsort_key_order_bits64 if kind == "f64" else ls.lib.labsort_key_order_bits
        assert int(U.image(np.array([w], dtype=x.dtype), kind)[0]) == f(int(w), ls.KEY[kind])
    # consecutive mode: neighbouring NaNs of different payloads are one run
    y = np.array([nans[0], nans[1], nans[2], pz, mz, mz, nans[3]], dtype=x.dtype)
    values, counts, first, inverse, m = U.expected(y, kind, consecutive=True)
    assert [int(v) for v in values] == [canon, pz, mz, canon] and list(counts) == [3, 1, 2, 1] and list(first) == [0, 3, 4, 6]


@pytest.mark.parametrize("kind", U.INT_KINDS)
@pytest.mark.parametrize("V", [1, 7, 1000])
def test_spread_closed_form(kind, V):
    """spread_expected, which sorts V values, against expected(), which sorts all n; the V values are
    distinct and, from V = 1000 on, differ in every byte of the word."""
    b = U.spread_values(V, kind)
    assert np.unique(b).size == V and b.dtype == U.word_dtype(kind)
    if V == 1000:
        for byte in range(b.dtype.itemsize):
            assert np.unique((b >> b.dtype.type(8 * byte)) & b.dtype.type(0xFF)).size > 200
    for n in sorted({1, max(V - 1, 1), V, V + 1, 10 * V + 3}):
        x = U.spread(n, V, kind)
        assert x.size == n and x.dtype == U.word_dtype(kind)
        np.testing.assert_array_equal(x, b[np.arange(n) % V])
        want, got = U.expected(x, kind), U.spread_expected(n, V, kind)
        assert got[4] == want[4] == min(V, n)
        for name, g, w in zip(("values", "counts", "first", "inverse"), got, want):
            assert g.dtype == w.dtype, name
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: n={n} V={V} {kind}")
    with pytest.raises(ValueError):
        U.spread_values(V, "f32")


def test_route_sizes():
    ids, ns = zip(*U.route_sizes(16384, 32768, 1 << 16, 1 << 18))
    assert ids[:3] == ("pair_tile-1", "pair_tile", "pair_tile+1") and ns[:3] == (16383, 16384, 16385)
    assert len(set(ids)) == len(set(ns)) == 12 and ns[-3:] == ((1 << 18) - 1, 1 << 18, (1 << 18) + 1)


def test_sweep_is_reproducible(ls):
    C = ls.unique_chunk_keys()
    a, b = list(U.sweep_cases(0x7171, C)), list(U.sweep_cases(0x7171, C))
    assert len(a) == 40 and a == b
    assert {c["kind"] for c in a} == set(U.KINDS) and {c["gen"] for c in a} == set(U.GENERATORS)
    assert {c["consecutive"] for c in a} == {False, True} and len({c["outputs"] for c in a}) >= 6
    assert U.expected(np.zeros(0, dtype=np.uint32), "u32")[4] == 0
