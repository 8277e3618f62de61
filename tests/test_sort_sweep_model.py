"""tests/sort_sweep_model.py on the host: the digit-mask rows hold exactly the mask they were asked
for and only images of words, the lone key sits where its variant says, and the committed seeds of
the three sweeps reach every class, path and option the GPU tests are meant to run.  The shapes of
the kernels come from the library's host getters; nothing here launches a kernel."""
import numpy as np
import pytest

import rowsort_model as R
import sort_sweep_model as S
import topk_model as T

COLS = [1, 2, 63, 64, 65, 300, 5000]
BOTH = [False, True]


@pytest.mark.parametrize("variant", S.VARIANTS)
@pytest.mark.parametrize("descending", BOTH)
@pytest.mark.parametrize("kind", R.KINDS)
def test_digit_mask_rows(kind, descending, variant):
    masks = S.masks_of(kind)
    assert len(masks) == (4 if R.is16(kind) else 16)
    for cols in COLS:
        x = S.digit_mask_rows(masks, cols, 0xD000 + cols, kind, descending, variant)
        assert x.shape == (len(masks), cols) and x.dtype == R.wdtype(kind)
        u = T.u_of(x, kind, descending)
        np.testing.assert_array_equal(u, R.u_of(x, kind, descending))  # the two models' images agree
        np.testing.assert_array_equal(T.u_of(T.raw_of(u, kind, descending), kind, descending), u)
        top = u >> u.dtype.type(8 * (u.dtype.itemsize - 1))
        assert bool(((top >= T.TOP_LO) & (top < T.TOP_HI)).all())  # no NaN, no image without a word
        want = [0] * len(masks) if cols == 1 else masks
        np.testing.assert_array_equal(S.mask_of(u), want, err_msg=f"{kind} cols={cols} {variant} descending={descending}")
        # the direction complements the image: the same digits differ in the other direction
        np.testing.assert_array_equal(S.mask_of(T.u_of(x, kind, not descending)), want)


@pytest.mark.parametrize("kind", R.KINDS)
def test_onebit_digits_take_two_values_one_bit_apart(kind):
    masks = S.masks_of(kind)
    for cols in COLS[1:]:
        u = T.u_of(S.digit_mask_rows(masks, cols, 0xD100 + cols, kind, False, "onebit"), kind, False)
        for r, m in enumerate(masks):
            for i in range(S.ndigits(kind)):
                vals = np.unique((u[r] >> u.dtype.type(8 * i)) & u.dtype.type(0xFF))
                if (m >> i) & 1:
                    assert vals.size == 2 and bin(int(vals[0]) ^ int(vals[1])).count("1") == 1, (kind, cols, m, i, vals)
                else:
                    assert vals.size == 1


@pytest.mark.parametrize("variant", ["lone_first", "lone_last", "lone_mid"])
@pytest.mark.parametrize("descending", BOTH)
@pytest.mark.parametrize("kind", R.KINDS)
def test_lone_key(kind, descending, variant):
    """All keys equal but the one at lone_position(): it differs from them in every masked digit and
    in no other, and is smaller than the rest (in the order asked for) in even rows, larger in odd ones."""
    masks = S.masks_of(kind)
    nd = S.ndigits(kind)
    for cols in COLS[1:]:
        seed = 0xD200 + cols
        u = T.u_of(S.digit_mask_rows(masks, cols, seed, kind, descending, variant), kind, descending)
        for r, m in enumerate(masks):
            at = S.lone_position(variant, cols, seed, r)
            assert at == {"lone_first": 0, "lone_last": cols - 1}.get(variant, at) and 0 <= at < cols
            if variant == "lone_mid" and cols >= 3:
                assert 0 < at < cols - 1
            rest = np.delete(u[r], at)
            assert bool((rest == rest[0]).all())
            x = int(u[r, at]) ^ int(rest[0])
            assert sum(((x >> (8 * i)) & 0xFF) != 0 for i in range(nd) if (m >> i) & 1) == bin(m).count("1")
            assert S.mask_of(u[r:r + 1])[0] == m
            if m:
                assert (int(u[r, at]) < int(rest[0])) == (r % 2 == 0)
    # lone_mid is not always the same place
    assert len({S.lone_position("lone_mid", 5000, 1, r) for r in range(16)}) > 8


def test_mask_matrix_and_segments():
    for kind, nrows in (("i32", 80), ("bf16", 20)):
        x, labels = S.mask_matrix(kind, 200, 0xD300)
        assert x.shape == (nrows, 200) and len(labels) == nrows
        np.testing.assert_array_equal(S.mask_of(T.u_of(x, kind)), [m for m, _ in labels])
        assert {v for _, v in labels} == set(S.VARIANTS)
    keys, offs, labels = S.mask_segments("f32", 16384, 0xD301)
    assert offs[0] == 0 and int(offs[-1]) == keys.size < 4_000_000 and len(labels) == offs.size - 1
    assert len(labels) == 16 * (5 * len(S.MASK_SEGMENT_LENGTHS) + len(S.TILE_VARIANTS))
    assert any(int(o) % 4 for o in offs[:-1])
    u = T.u_of(keys, "f32")
    for (a, b), (length, m, v) in zip(zip(offs[:-1], offs[1:]), labels):
        assert int(b) - int(a) == length
        assert S.mask_of(u[None, int(a):int(b)])[0] == (m if length > 1 else 0)
    assert S.mask_segments("u32", 32768, 0xD302)[0].size < 4_000_000


def test_sweep_rows_by_name():
    rng = np.random.default_rng(5)
    for kind in R.KINDS:
        for gen in S.PLAIN_GENS + ("mask:1:onebit", "mask:2:lone_mid", "mask:3:full", "mask:0:full"):
            for cols in (1, 2, 70):
                x = S.sweep_row(gen, cols, kind, True, rng)
                assert x.shape == (cols,) and x.dtype == R.wdtype(kind), (kind, gen)
                u = R.u_of(x, kind, True).astype(np.int64)
                if gen == "sorted":
                    assert bool((np.diff(u) >= 0).all())
                if gen == "reversed":
                    assert bool((np.diff(u) <= 0).all())
                if gen.startswith("mask:") and cols > 1:
                    assert S.mask_of(R.u_of(x, kind, True)[None])[0] == int(gen.split(":")[1])
                if gen in ("all_equal", "all_nan", "mask:0:full"):
                    assert S.mask_of(R.u_of(x, kind, True)[None])[0] == 0


# ---- what the committed seeds reach ----

def shapes(ls):
    e = ls.segment_class_edges(False)
    return e[:-1], ls.segment_tile_keys(), ls.segment_pair_tile_keys()


def test_rowsort_sweep_coverage(ls):
    edges, tile, pair_tile = shapes(ls)
    assert edges == ls.segment_class_edges(True)[:-1]  # one set of classes below the tiles
    cases = [c for seed in S.ROWSORT_SEEDS for c in S.rowsort_sweep_cases(seed, edges, tile, pair_tile)]
    assert len(cases) == len(S.ROWSORT_SEEDS) * S.ROWSORT_CASES == 120
    on_edge = 0
    for c in cases:
        assert c["x"].shape == (c["rows"], c["cols"]) and c["x"].dtype == R.wdtype(c["kind"])
        assert 1 <= c["rows"] <= 48 and 1 <= c["cols"] <= 40000 and c["rows"] * c["cols"] <= 1 << 19
        assert R.is16(c["kind"]) or (c["in_off"], c["out_off"]) == (0, 0)
        assert len(c["gens"]) == c["rows"]
        on_edge += any(abs(c["cols"] - e) <= 1 for e in [64] + edges + [pair_tile, tile])
    assert on_edge >= len(cases) // 3
    reached = {(R.is16(c["kind"]), c["with_idx"], c["path"]) for c in cases}
    for wide16 in BOTH:
        for with_idx in BOTH:
            for path in ["short", "long"] + [f"class{k}" for k in range(5)]:
                assert (wide16, with_idx, path) in reached, (wide16, with_idx, path)
    assert {c["kind"] for c in cases} == set(R.KINDS)
    assert {c["grid"] for c in cases if c["path"].startswith("class")} == set(S.GRIDS)
    assert {c["descending"] for c in cases} == {False, True}
    assert {(c["in_off"], c["out_off"]) for c in cases if R.is16(c["kind"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # every mask of each width, in rows that an LDS class kernel's pass loop sorts, read back from the words
    seen = {16: set(), 32: set()}
    variants = set()
    for c in cases:
        if c["path"].startswith("class"):
            got = S.mask_of(T.u_of(c["x"], c["kind"], c["descending"]))
            for g, m in zip(c["gens"], got):
                if g.startswith("mask:"):
                    assert int(g.split(":")[1]) == m, c["tag"]
                    seen[T.bits_of(c["kind"])].add(int(m))
                    variants.add(g.split(":")[2])
    assert seen[16] == set(range(4)) and seen[32] == set(range(16)), seen
    assert variants == set(S.VARIANTS)
    assert {g for c in cases for g in c["gens"] if not g.startswith("mask:")} == set(S.PLAIN_GENS)
    assert len({c["tag"] for c in cases}) == len(cases)


def test_sort16_sweep_coverage(ls):
    C, tile = ls.sort16_chunk_keys(), ls.segment_tile_keys()
    cases = [c for seed in S.SORT16_SEEDS for c in S.sort16_sweep_cases(seed, C, tile)]
    assert len(cases) == len(S.SORT16_SEEDS) * S.SORT16_CASES == 48
    for c in cases:
        assert c["x"].shape == (c["rows"], c["cols"]) and c["x"].dtype == np.uint16
        assert 1 <= c["rows"] <= 4 and tile < c["cols"] <= 6 * C
        if c["edge"]:
            assert (c["cols"] + 1) % C <= 2
    assert sum(c["edge"] is not None for c in cases) == len(cases) // 2
    assert {c["entry"] for c in cases} == set(S.ENTRIES)
    assert {c["edge"] for c in cases} == {None, "mC-1", "mC", "mC+1"}
    assert {c["kind"] for c in cases} == {"bf16", "f16"}
    assert {(c["descending"], c["with_idx"]) for c in cases} == {(a, b) for a in BOTH for b in BOTH}
    assert {(c["in_off"], c["out_off"]) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {int(g.split(":")[1]) for c in cases for g in c["gens"] if g.startswith("mask:")} == set(range(4))


def test_f32_segment_sweep_coverage(ls):
    _, tile, pair_tile = shapes(ls)
    cases = [c for seed in S.F32SEG_SEEDS for c in S.f32_segment_sweep_cases(seed, tile, pair_tile)]
    assert len(cases) == len(S.F32SEG_SEEDS) * S.F32SEG_CASES == 180
    for c in cases:
        offs = c["offs"].astype(np.int64)
        assert c["n"] <= 1 << 17 and c["keys"].shape == (c["n"],) and offs.size == c["nseg"] + 1
        assert offs[0] == 0 and offs[-1] == c["n"] and bool((np.diff(offs) >= 0).all())
        assert c["m"] in (0, c["true_max"]) and (c["vals"] is not None) == c["pairs"]
        assert (c["path"] == "lds") == (0 < c["m"] <= (pair_tile if c["pairs"] else tile))
    reached = {(c["path"], c["pairs"], c["inplace"]) for c in cases}
    assert reached == {(p, a, b) for p in ("lds", "general") for a in BOTH for b in BOTH}
    assert any(bool((np.diff(c["offs"].astype(np.int64)) == 0).any()) for c in cases)  # empty segments
    assert any(c["path"] == "lds" and c["true_max"] > 4096 for c in cases)  # the tile class
    assert any(c["path"] == "general" and c["m"] > 0 for c in cases)  # a true promise past the tile
    lds_gens = {g for c in cases if c["path"] == "lds" for g in c["gens"]}
    assert {int(g.split(":")[1]) for g in lds_gens if g.startswith("mask:")} == set(range(16))
    assert {"all_nan", "ties"} <= lds_gens
