"""CPU tests of the top-p filter's rule: the model (tests/top_p_model.py) against float64 arithmetic, its
two forms against each other, and labsort_top_p_weight (a host function: nothing is launched) against
the model."""
import numpy as np
import pytest

import rowsort_model as R
import top_p_model as P

KINDS = pytest.mark.parametrize("kind", P.KINDS)
# 0, -0.0, 1, 1.5, +inf, -inf, NaNs, 2^-40, its predecessor, the smallest subnormal, 2^-126, its
# neighbours, the last value below 1, 2^-17 (the first weight that uses the shift by zero's neighbour)
F32_EDGES = np.array([0x00000000, 0x80000000, 0x3F800000, 0x3FC00000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
                      0x7F800001, 0x2B800000, 0x2B7FFFFF, 0x00000001, 0x00800000, 0x007FFFFF, 0x00800001, 0x3F7FFFFF,
                      0x37000000, 0x36FFFFFF, 0x1F800000, 0x1F7FFFFF, 0x80000001, 0xBF800000], dtype=np.uint32)


def float64_weight(x, kind):
    """floor(clamp(x) 2^40) in float64, which holds x 2^40 exactly for every float32 x in [0, 1]."""
    neg = (P.widen(x, kind) >> np.uint32(31)) != 0
    with np.errstate(invalid="ignore"):  # (signalling NaNs)
        v = P.widen(x, kind).view(np.float32).astype(np.float64)
        c = np.where(np.isnan(v) | neg, 0.0, np.minimum(v, 1.0))
    return np.floor(c * float(P.ONE)).astype(np.uint64)


def all_words(kind):
    if kind == "f32":
        rng = np.random.default_rng(0x70B0)
        return np.concatenate([F32_EDGES, rng.integers(0, 1 << 32, size=60000, dtype=np.uint64).astype(np.uint32),
                               # exponents around the weights that matter: 2^-41 .. 2
                               (rng.integers(85, 129, size=60000, dtype=np.uint64) << np.uint64(23)
                                | rng.integers(0, 1 << 23, size=60000, dtype=np.uint64)).astype(np.uint32)])
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


@KINDS
def test_weight_from_bits_is_the_float64_floor(kind):
    x = all_words(kind)
    np.testing.assert_array_equal(P.weight(x, kind), float64_weight(x, kind))


def test_weight_edges():
    w = P.weight(F32_EDGES, "f32").tolist()
    assert w[:11] == [0, 0, P.ONE, P.ONE, P.ONE, 0, 0, 0, 0, 1, 0]
    assert w[11:16] == [0, 0, 0, 0, P.ONE - (1 << 16)]
    assert P.weight(np.array([0x3C00, 0x3BFF, 0x0001, 0x7C00, 0xFC00, 0x7E00, 0x8000], dtype=np.uint16), "f16").tolist() == \
        [P.ONE, P.ONE - (1 << 29), 1 << 16, P.ONE, 0, 0, 0]
    assert P.weight(np.array([0x3F80, 0x3F7F, 0x7F80, 0x7FC0, 0x8000, 0x2B80, 0x2B7F], dtype=np.uint16), "bf16").tolist() == \
        [P.ONE, P.ONE - (1 << 32), P.ONE, 0, 0, 1, 0]


@KINDS
def test_library_weight_equals_the_model(ls, kind):
    x = all_words(kind)
    want = P.weight(x, kind)
    got = np.array([ls.top_p_weight(int(v), kind) for v in x.tolist()], dtype=np.uint64)
    np.testing.assert_array_equal(got, want)
    for other in ("u32", "i32", "u64", "i64", "f64"):
        assert ls.top_p_weight(0x3F800000, other) == 0


def test_fixed_p_and_target():
    assert P.fixed_p(1.0) == (1 << 32, False) and P.fixed_p(0.5) == (1 << 31, False)
    assert P.fixed_p(2.0 ** -30) == (4, False) and P.fixed_p(2.0 ** -40) == (1, False) and P.fixed_p(1e-45) == (1, False)
    assert P.fixed_p(0.0) == (1, True) and P.fixed_p(-0.0) == (1, True) and P.fixed_p(-1.0) == (1, True)
    assert P.fixed_p(1.5) == (1 << 32, True) and P.fixed_p(float("nan")) == (1 << 32, True)
    assert P.fixed_p(float("inf")) == (1 << 32, True) and P.fixed_p(float("-inf")) == (1, True)
    assert P.fixed_p(np.float32(0.9))[0] == int(np.floor(float(np.float32(0.9)) * 2.0 ** 32))
    assert P.target(1 << 32, 12345) == 12345 and P.target(1, 1) == 1 and P.target(1 << 31, 3) == 2
    assert P.target(1, (1 << 63) - 1) == 1 << 31 and P.target(3, 1 << 32) == 3 and P.target(3, (1 << 32) + 1) == 4


@KINDS
@pytest.mark.parametrize("cols", [1, 2, 65, 1000, 20000])
def test_the_two_forms_agree(cols, kind):
    x = P.special_rows(kind, cols, 0x70B1 + cols)
    for p in (2.0 ** -30, 0.5, 0.9, 1.0, np.array([0.3, 1.0, 0.7, 0.999], dtype=np.float32),
              np.array([0.0, -1.0, 1.5, np.nan], dtype=np.float32)):
        sk, sm, sks, sflag = P.by_scan(x, p, kind, 7)
        tk, tm, tks, tflag = P.by_threshold(x, p, kind, 7)
        np.testing.assert_array_equal(sks, tks)
        np.testing.assert_array_equal(sm, tm)
        np.testing.assert_array_equal(sk, tk)
        assert sflag and tflag  # row 2 has no mass
        np.testing.assert_array_equal(sm.sum(axis=1), sks)
        assert sks[2] == cols
    if cols >= 1000:  # (a shorter row may hold planted values alone)
        assert not P.kept_counts(x[:2], 0.5, kind)[1]


@KINDS
def test_kept_count_is_monotone_in_p(kind):
    x = P.special_rows(kind, 3000, 0x70B2)[:2]
    exp = R.expected(x, True, kind)
    ps = np.sort(np.concatenate([np.random.default_rng(0x70B3).random(60).astype(np.float32),
                                 np.array([2.0 ** -32, 2.0 ** -30, 0.5, 1.0], dtype=np.float32)]))
    ks = np.stack([P.kept_counts(x, p, kind, exp)[0] for p in ps])
    assert bool((np.diff(ks, axis=0) >= 0).all())
    assert bool((ks >= 1).all()) and bool((ks[-1] == np.count_nonzero(P.weight(x, kind), axis=1) + np.count_nonzero(
        R.u_of(x, kind, True) == R.u_of(np.array([[R.nan_word(kind)]], dtype=x.dtype), kind, True)[0, 0], axis=1)).all())


@KINDS
@pytest.mark.parametrize("cols", [50257, 151936])
def test_kept_count_lies_in_the_float64_band(cols, kind):
    """With m(n) the float64 mass of the first n sorted entries and M = m(cols): m(k) >= p M - e and
    m(k - 1) < p M + e, e = 2^-32 M + cols 2^-40: the truncation of P and of the weights."""
    for temperature in (1.0, 0.7):
        x = P.softmax_words(cols, kind, 0x70B4 + cols, temperature)
        exp = R.expected(x, True, kind)
        vals = P.widen(exp[0], kind).view(np.float32).astype(np.float64)
        m = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(vals, axis=1)], axis=1)
        for p in (0.1, 0.5, 0.9, 0.99, 0.999, 1.0):
            ks, flagged = P.kept_counts(x, p, kind, exp)
            assert not flagged
            pf = float(np.float32(p))
            for r in range(x.shape[0]):
                M, k = m[r, cols], int(ks[r])
                e = 2.0 ** -32 * M + cols * 2.0 ** -40
                assert 1 <= k <= cols
                assert m[r, k] >= pf * M - e and m[r, k - 1] < pf * M + e, (kind, cols, temperature, p, r, k)
