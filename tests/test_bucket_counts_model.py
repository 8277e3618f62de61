"""The numpy models of tests/bucket_counts_model.py against the definitions, one comparison at a time,
on small cases; every row of counts sums to nv.  No library call."""
import numpy as np
import pytest

import bucket_counts_model as BM
import searchsorted_model as SM


@pytest.mark.parametrize("kind", SM.KINDS)
def test_counts_match_the_double_loop(kind):
    for gen, nedges, nv in (("random", 0, 9), ("random", 1, 30), ("random", 2, 30), ("random", 37, 200), ("equal", 20, 90),
                            ("two", 33, 150), ("runs:5", 64, 250)):
        edges, vals, _, _ = SM.shared_case(gen, nedges, nv, 0xB0C + nedges, kind)
        for right in (False, True):
            got = BM.expected(edges, vals, right, kind)
            assert got.dtype == np.uint32 and got.shape == (nedges + 1,)
            np.testing.assert_array_equal(got, BM.loop_counts(edges, vals, right, kind), err_msg=f"{kind} {gen} {nedges} {right}")
            assert int(got.sum()) == nv


@pytest.mark.parametrize("kind", SM.FLOATS)
def test_specials_fall_where_the_contract_says(kind):
    """Every NaN lands in the last bin unless an edge is a NaN; -0.0 and +0.0 are two values."""
    s = SM.float_specials(kind)
    zeros = SM.from_image(SM.image(np.array([0], dtype=SM.word_dtype(kind)), kind), kind)  # +0.0
    neg0 = np.array([1 << (8 * SM.esz(kind) - 1)], dtype=SM.word_dtype(kind))
    edges = SM.ascending(np.concatenate([zeros, neg0]), kind)  # (-0.0, +0.0)
    assert edges[0] == neg0[0]
    for right in (False, True):
        got = BM.expected(edges, s, right, kind)
        np.testing.assert_array_equal(got, BM.loop_counts(edges, s, right, kind))
        assert int(got.sum()) == s.size
    # left: -0.0 goes below the first edge, +0.0 between the two; right: one bin up each
    np.testing.assert_array_equal(BM.expected(edges, np.concatenate([neg0, zeros]), False, kind), [1, 1, 0])
    np.testing.assert_array_equal(BM.expected(edges, np.concatenate([neg0, zeros]), True, kind), [0, 1, 1])
    nan = s[SM.image(s, kind) == np.iinfo(SM.word_dtype(kind)).max]
    assert nan.size >= 2
    np.testing.assert_array_equal(BM.expected(edges, nan, False, kind), [0, 0, nan.size])


@pytest.mark.parametrize("kind", ["u32", "f16", "i64"])
def test_rows_and_sums(kind):
    edges, vals, left, right = SM.row_case("random", 3, 50, 333, 0xB1, kind)
    for r, ranks in ((False, left), (True, right)):
        got = BM.expected(edges, vals, r, kind)
        assert got.shape == (3, 51)
        np.testing.assert_array_equal(got.sum(axis=1), [333] * 3)
        for i in range(3):
            np.testing.assert_array_equal(got[i], BM.loop_counts(edges[i], vals[i], r, kind))
            np.testing.assert_array_equal(got[i], np.bincount(ranks[i], minlength=51))
    # one edge row for every row of the values
    got = BM.expected(edges[0], vals, False, kind)
    for i in range(3):
        np.testing.assert_array_equal(got[i], BM.loop_counts(edges[0], vals[i], False, kind))
    assert BM.expected(edges[0], vals[:0], False, kind).shape == (0, 51)


def test_sweep_cases_sum_to_nv():
    cases = [c for c in SM.sweep_cases(0xB2, {k: 4096 for k in SM.KINDS}, 512, count=12) if not c["sorter"]]
    assert cases
    for c in cases:
        seq, vals, _, ranks = SM.sweep_case(c)
        got = BM.counts_of_ranks(ranks, c["cols"])
        np.testing.assert_array_equal(got, BM.expected(seq, vals, c["right"], c["kind"]))
        np.testing.assert_array_equal(got.sum(axis=-1), np.full(vals.shape[0], c["nv"]))


@pytest.mark.parametrize("kind", BM.BIN_KINDS)
def test_bincount_model(kind):
    for nbins in (0, 1, 2, 255, 1000):
        x = BM.bincount_words(700, nbins, 0xB3, kind)
        got = BM.bincount_expected(x, nbins, kind)
        assert got.dtype == np.uint32 and got.shape == (nbins + 1,) and int(got.sum()) == 700
        np.testing.assert_array_equal(got, BM.bincount_loop(x, nbins, kind))
        if nbins:
            assert got[nbins] > 0 and got[:nbins].sum() > 0
        rows = np.stack([x, x[::-1], np.roll(x, 1)])
        np.testing.assert_array_equal(BM.bincount_expected(rows, nbins, kind), np.stack([got] * 3))
    # a negative value of a signed kind is outside; the same word of the unsigned kind is a large value: outside too
    w = np.array([0xFFFFFFFF if kind in ("u32", "i32") else 0xFFFFFFFFFFFFFFFF, 3], dtype=SM.word_dtype(kind))
    np.testing.assert_array_equal(BM.bincount_expected(w, 5, kind), [0, 0, 0, 1, 0, 1])
