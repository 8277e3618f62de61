"""CPU tests of tests/searchsorted_model.py, the numpy statement of labsort_searchsorted_device's
contract: the model against the definition counted one comparison at a time, against np.searchsorted
on raw NaN-free keys, and the NaN and signed-zero rules.  Nothing here calls the library."""
import numpy as np
import pytest

import searchsorted_model as SM

ALL = pytest.mark.parametrize("kind", SM.KINDS)
NATIVE = {"u32": np.uint32, "i32": np.int32, "f32": np.float32, "f16": np.float16, "u64": np.uint64, "i64": np.int64,
          "f64": np.float64}


@ALL
def test_model_against_a_plain_loop(kind):
    for gen in ("random", "equal", "two", "few", "runs:3"):
        for cols in (0, 1, 2, 3, 17, 64):
            seq = SM.sequence(gen, cols, 11, kind)
            assert seq.size == cols and bool((np.diff(SM.image(seq, kind).astype(np.float64)) >= 0).all())
            vals = SM.probes(seq, kind) if cols else SM.random_words(9, 3, kind)
            for right in (False, True):
                got = SM.expected(seq, vals, right, kind)
                assert got.dtype == np.uint32 and np.array_equal(got, SM.loop_ranks(seq, vals, right, kind)), (gen, cols)
                assert int(got.max()) <= cols


@ALL
def test_sorter_and_row_forms(kind):
    rng = np.random.default_rng(5)
    raw = np.stack([SM.random_words(40, 20 + r, kind) for r in range(3)])
    order = np.argsort(SM.image(raw, kind), axis=-1, kind="stable")
    seq = np.take_along_axis(raw, order, axis=-1)
    vals = np.stack([SM.probes(raw[r], kind)[:100] for r in range(3)])
    for right in (False, True):
        want = SM.expected(seq, vals, right, kind)
        assert np.array_equal(SM.expected(raw, vals, right, kind, sorter=order.astype(np.uint32)), want)
        for r in range(3):
            assert np.array_equal(want[r], SM.loop_ranks(seq[r], vals[r], right, kind))
            # one shared sequence, values of any shape
            assert np.array_equal(SM.expected(seq[r], vals, right, kind)[1], SM.loop_ranks(seq[r], vals[1], right, kind))
            assert np.array_equal(SM.expected(raw[r], vals[r], right, kind, sorter=order[r]), want[r])
    assert rng is not None


@pytest.mark.parametrize("kind", sorted(NATIVE))
def test_model_is_numpy_searchsorted_on_raw_keys(kind):
    """On keys free of NaNs and of zeros of both signs the image order is the keys' own."""
    rng = np.random.default_rng(17)
    nat = NATIVE[kind]
    if kind in SM.FLOATS:
        a = (rng.standard_normal(500) * 100).astype(nat)
        v = np.concatenate([a[:200], (rng.standard_normal(300) * 100).astype(nat)])
        a, v = a[a != 0], v[v != 0]
    else:
        info = np.iinfo(nat)
        a = rng.integers(info.min, info.max, size=500, dtype=nat, endpoint=True)
        v = np.concatenate([a[:200], rng.integers(info.min, info.max, size=300, dtype=nat, endpoint=True),
                            np.array([info.min, info.max], dtype=nat)])
    a = np.sort(a)
    words = lambda t: np.ascontiguousarray(t).view(SM.word_dtype(kind))  # noqa: E731
    for right in (False, True):
        want = np.searchsorted(a, v, side="right" if right else "left").astype(np.uint32)
        assert np.array_equal(SM.expected(words(a), words(v), right, kind), want)


@pytest.mark.parametrize("kind", SM.FLOATS)
def test_nan_and_signed_zero_rules(kind):
    s = SM.float_specials(kind)
    u = SM.image(s, kind)
    dt = SM.word_dtype(kind)
    top, bits = np.iinfo(dt).max, 8 * SM.esz(kind)
    sign = dt(1 << (bits - 1))
    mag = {"f32": 0x7F800000, "bf16": 0x7F80, "f16": 0x7C00, "f64": 0x7FF0000000000000}[kind]
    nan = (s & ~sign) > dt(mag)
    assert int(nan.sum()) >= 4 and bool((u[nan] == top).all()) and bool((u[~nan] < top).all())  # one value, past every number
    seq = SM.ascending(s, kind)
    n, k = seq.size, int(nan.sum())
    for w in s[nan]:
        assert SM.expected(seq, np.array([w], dtype=dt), False, kind)[0] == n - k
        assert SM.expected(seq, np.array([w], dtype=dt), True, kind)[0] == n
    pinf = np.array([mag], dtype=dt)
    assert SM.expected(seq, pinf, True, kind)[0] == n - k  # +inf is the last number
    # -0.0 < +0.0: two values, next to each other
    zeros = np.array([sign, 0], dtype=dt)
    assert int(SM.image(zeros, kind)[0]) + 1 == int(SM.image(zeros, kind)[1])
    both = SM.ascending(np.array([0, sign, 0, sign, sign], dtype=dt), kind)
    assert np.array_equal(SM.expected(both, zeros, False, kind), [0, 3])
    assert np.array_equal(SM.expected(both, zeros, True, kind), [3, 5])


def test_sizes_and_sweep_are_what_the_gpu_tests_assume():
    assert SM.cols_sizes(16384)[-7:] == [20479, 20480, 20481, 24575, 24576, 24577, 3 * (1 << 20) + 5]
    assert SM.nv_sizes(4096) == [1, 7, 8, 9, 4095, 4096, 4097, 12293]
    L = {k: 65536 // SM.esz(k) for k in SM.KINDS}
    cases = list(SM.sweep_cases(91, L, 4096))
    assert len(cases) == 40 and cases == list(SM.sweep_cases(91, L, 4096))
    assert {c["kind"] for c in cases} == set(SM.KINDS)
    for key in ("right", "sorter", "per_row"):
        assert {c[key] for c in cases} == {False, True}
    assert any(c["cols"] > L[c["kind"]] for c in cases) and any(c["cols"] <= L[c["kind"]] for c in cases)
    for c in cases[:6]:
        seq, vals, sorter, want = SM.sweep_case(c)
        assert vals.shape == (c["rows"], c["nv"]) == want.shape and int(want.max()) <= c["cols"]
        assert (sorter is not None) == c["sorter"] and seq.ndim == (2 if c["per_row"] else 1)


@ALL
def test_long_run_sequences_tie_consecutive_samples(kind):
    """runs:<len> and few give runs that cover whole strides of a long sequence's sample table."""
    L = 65536 // SM.esz(kind)
    cols = L + 1 + SM.SAMPLES
    stride = (cols + SM.SAMPLES - 1) // SM.SAMPLES
    for ln in (stride - 1, stride + 1, 3 * stride + 5):
        seq = SM.sequence(f"runs:{ln}", cols, 3, kind)
        u = SM.image(seq, kind)
        assert bool((u[1:] >= u[:-1]).all())
        ends = u[np.minimum(np.arange(1, SM.SAMPLES + 1) * stride, cols) - 1]
        if ln > stride:
            assert int((ends[1:] == ends[:-1]).sum()) > 0
