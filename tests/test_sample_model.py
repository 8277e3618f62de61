"""CPU tests of tests/sample_model.py, the numpy model of labsort_sample_device's contract: the model
against a plain loop, the words at which the draw moves from one element to the next, the ends of the
word range, exact word counts, and the elements that are never drawn."""
import numpy as np
import pytest

import rowsort_model as R
import sample_model as M
import top_p_model as P

KINDS = pytest.mark.parametrize("kind", P.KINDS)


def loop_draw(x_row, U, kind):
    """One draw by a loop over the row in Python integers; None for a row without mass."""
    w = [int(v) for v in P.weight(np.asarray(x_row), kind)]
    W = sum(w)
    if W == 0:
        return None
    s, run = (int(U) * W) >> 32, 0
    for j, wj in enumerate(w):
        run += wj
        if run > s:
            return j
    raise AssertionError("s < W")


def ends_at(x_row, kind):
    """{cumulative mass: the position of the weighted element that ends there}."""
    w = P.weight(np.asarray(x_row), kind)
    cum = np.cumsum(w, dtype=np.uint64)
    return {int(c): j for j, c in enumerate(cum) if w[j]}


@KINDS
def test_the_model_is_the_plain_loop(kind):
    rng = np.random.default_rng(0x5A30)
    for cols in (1, 2, 9, 300):
        x = np.concatenate([P.special_rows(kind, cols, 0x5A31 + cols), P.softmax_words(cols, kind, 0x5A32 + cols, 0.7)])
        U = rng.integers(0, 1 << 32, size=(x.shape[0], 40), dtype=np.uint64)
        U[:, 0], U[:, 1] = 0, 0xFFFFFFFF
        got, flagged = M.draw(x, U, kind)
        assert got.dtype == np.uint32 and got.shape == U.shape
        nomass = [r for r in range(x.shape[0]) if not P.weight(x[r], kind).any()]
        assert flagged == bool(nomass)
        for r in range(x.shape[0]):
            for d in range(U.shape[1]):
                want = loop_draw(x[r], U[r, d], kind)
                assert int(got[r, d]) == (M.SENTINEL if want is None else want), (kind, cols, r, d)


@KINDS
def test_boundaries_are_where_the_draw_moves(kind):
    """At U_b - 1 the draw is the element that ends at c, at U_b the next element with a weight.  (Rows
    of a few hundred sizeable weights: every element has words of its own, so no two c share a U_b.)"""
    for cols in (2, 9, 257):
        x = P.softmax_words(cols, kind, 0x5A33 + cols, rows=1)[0].copy()
        x[cols // 2] = 0  # (a weightless element inside the row)
        ub, cs = M.boundaries(x, kind)
        end = ends_at(x, kind)
        weighted = sorted(end.values())
        assert len(ub) == len(weighted) - 1 and len(set(ub)) == len(ub) and all(0 < u < (1 << 32) for u in ub)
        U = np.array([[u - 1 for u in ub] + list(ub)], dtype=np.uint64)
        got = M.draw(x.reshape(1, -1), U, kind)[0][0]
        for i, c in enumerate(cs):
            j = end[c]
            assert int(got[i]) == j
            assert int(got[len(ub) + i]) == weighted[weighted.index(j) + 1]


@KINDS
def test_the_ends_of_the_word_range(kind):
    x = P.special_rows(kind, 300, 0x5A34)[[0, 1, 3]]
    x[:, :3], x[:, -3:] = 0, 0  # leading and trailing runs without weight
    got, flagged = M.draw(x, np.array([[0, 0xFFFFFFFF]] * 3, dtype=np.uint64), kind)
    assert not flagged
    for r in range(3):
        nz = np.flatnonzero(P.weight(x[r], kind))
        assert int(got[r, 0]) == nz[0] >= 3 and int(got[r, 1]) == nz[-1] < 297


@KINDS
def test_exact_word_counts_of_a_dyadic_row(kind):
    """Weights 1/2, 1/4, 1/8, 1/8: the four ranges of U hold exactly 2^31, 2^30, 2^29 and 2^29 words."""
    x = P.words_of(np.array([0.5, 0.25, 0.125, 0.125]), kind)
    ub, cs = M.boundaries(x, kind)
    assert ub == [1 << 31, 3 << 30, 7 << 29]
    edges = [0] + ub + [1 << 32]
    assert [b - a for a, b in zip(edges, edges[1:])] == [1 << 31, 1 << 30, 1 << 29, 1 << 29]
    U = np.array([[e - 1 for e in edges[1:]] + edges[:-1]], dtype=np.uint64)
    assert M.draw(x.reshape(1, -1), U, kind)[0][0].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]


@KINDS
def test_a_weightless_position_is_never_drawn(kind):
    """NaNs, negatives, zeros and values below 2^-40, at random words and at every boundary."""
    rng = np.random.default_rng(0x5A35)
    for cols in (24, 300):
        x = P.special_rows(kind, cols, 0x5A36 + cols)
        w = P.weight(x, kind)
        assert not w[2].any() and (w[0] == 0).any() and (w[1] == 0).any()
        rows = []
        for r in (0, 1, 3):
            ub, _ = M.boundaries(x[r], kind)
            near = [u for b in ub for u in (b - 1, b) if 0 <= u < (1 << 32)]
            rows.append(near + rng.integers(0, 1 << 32, size=2 * cols + 64 - len(near), dtype=np.uint64).tolist())
        U = np.array(rows, dtype=np.uint64)
        got, flagged = M.draw(x[[0, 1, 3]], U, kind)
        assert not flagged
        for i, r in enumerate((0, 1, 3)):
            assert w[r][got[i].astype(np.int64)].all()
        got, flagged = M.draw(x[[2]], U[:1], kind)
        assert flagged and (got == M.SENTINEL).all()


@KINDS
def test_words_per_element_are_floor_or_ceil(kind):
    """The number of words that draw an element, from the boundaries, differs from w 2^32 / W by less
    than 1 (compared as integers: |n W - w 2^32| < W)."""
    for cols, seed in ((9, 1), (300, 2), (4097, 3)):
        x = P.special_rows(kind, cols, 0x5A37 + seed)[1]
        w = P.weight(x, kind)
        W = int(w.sum(dtype=np.uint64))
        ub, cs = M.boundaries(x, kind)
        end = ends_at(x, kind)
        edges = [0] + [min(u, 1 << 32) for u in ub] + [1 << 32]
        tops = cs + [W]
        assert len(tops) == len(end)
        for a, b, c in zip(edges, edges[1:], tops):
            n, wj = b - a, int(w[end[c]])
            assert n >= 0 and abs(n * W - (wj << 32)) < W, (kind, cols, c)
        assert sum(b - a for a, b in zip(edges, edges[1:])) == 1 << 32
