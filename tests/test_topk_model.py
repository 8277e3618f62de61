"""The host model of the radix select (tests/topk_model.py) against plain numpy: select_expected
equals the full stable argsort, narrow_level gives every generator's intended level, both sides of
the candidate buffer's capacity included, the constants are the header's, and the seeded sweep of
test_gpu_topk_select.py reaches every path and every narrowing level.  No GPU."""
import collections

import numpy as np
import pytest

import topk_model as T


def full(u, k):
    return np.argsort(u, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint16])
def test_select_expected_is_the_stable_argsort(dtype):
    rng = np.random.default_rng(0x70E0)
    top = np.iinfo(dtype).max
    for rows, cols in ((1, 1), (3, 2), (4, 257), (2, 5000)):
        arrays = {"random": rng.integers(0, int(top) + 1, size=(rows, cols), dtype=np.uint64).astype(dtype),
                  "heavy ties": rng.integers(0, 5, size=(rows, cols)).astype(dtype),
                  "all equal": np.full((rows, cols), 77, dtype=dtype),
                  "extremes": rng.choice(np.array([0, 1, top - 1, top], dtype=dtype), size=(rows, cols))}
        for name, u in arrays.items():
            for k in sorted({1, 2, cols // 2, cols - 1, cols} & set(range(1, cols + 1))):
                got = T.select_expected(u, k)
                assert got.shape == (rows, k)
                np.testing.assert_array_equal(got, full(u, k), err_msg=f"{name} {dtype.__name__} ({rows}, {cols}) k={k}")


@pytest.mark.parametrize("dtype", [np.uint32, np.uint16])
@pytest.mark.parametrize("at", ["first", "last"])
def test_select_expected_threshold_tie_at_the_row_ends(dtype, at):
    """The k-th key's ties begin at position 0, or end at cols - 1; k cuts the run of ties."""
    cols = 301
    u = (np.arange(cols, dtype=np.uint64) % 50 + 100).astype(dtype).reshape(1, cols)
    u[0, 7:12] = 3  # five keys below the tie value
    ties = [0, 20, 21, 150] if at == "first" else [20, 21, 150, cols - 1]
    u[0, ties] = 9
    for k in (6, 7, 8, 9):  # one to four of the ties taken
        got = T.select_expected(u, k)
        np.testing.assert_array_equal(got, full(u, k))
        assert list(got[0, 5:]) == ties[:k - 5]


def test_expected_keys_and_positions_per_kind():
    """expected() against the kinds' own models (full argsorts) on words with specials and ties."""
    import f16_model as M16
    import f32_model as M32
    for largest in (False, True):
        for k in (1, 9, 400):
            x = M32.random_words((3, 400), 5)
            x[1] = M32.tie_words((400,), 6)
            ek, ei = M32.topk_expected(x, k, largest)
            gk, gi = T.expected(x, k, "f32", largest)
            np.testing.assert_array_equal(gk, ek)
            np.testing.assert_array_equal(gi, ei)
            for kind, flip in (("u32", 0), ("i32", 0x80000000)):
                idx = full(x ^ np.uint32(flip ^ (0xFFFFFFFF if largest else 0)), k)
                gk, gi = T.expected(x, k, kind, largest)
                np.testing.assert_array_equal(gi, idx)
                np.testing.assert_array_equal(gk, np.take_along_axis(x, idx, axis=1))
            for kind in M16.KINDS:
                y = M16.random_words((3, 400), 7, kind)
                y[1] = M16.tie_words((400,), 8, kind)
                ek, ei = M16.topk_expected(y, k, largest, kind)
                gk, gi = T.expected(y, k, kind, largest)
                np.testing.assert_array_equal(gk, ek)
                np.testing.assert_array_equal(gi, ei)


def test_constants_are_the_headers():
    c = T.constants()
    assert set(c) == {"TK_CHUNK", "TK_BLOCK", "TK_CAND_DIV", "TK_MAX_HIST_WG"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    # the shapes test_gpu_topk_select.py is written for: its long row is the first with two chunks per
    # histogram workgroup and two steps of the scan, its matrix rows have a capacity of 8750
    assert c["TK_MAX_HIST_WG"] == c["TK_BLOCK"] == 1024 and c["TK_CHUNK"] == 16384 and c["TK_CAND_DIV"] == 8
    assert T.cap_of(70001, c) == 8750


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("largest", [False, True])
def test_generated_images_are_images_of_words(kind, largest):
    """raw_of and u_of are inverse on what the generators produce."""
    bits, cols = T.bits_of(kind), 20001
    rows = [T.row_narrowing_at(lv, cols, 3, bits) for lv in list(range(bits // 8 - 1)) + [T.NEVER]]
    rows += [T.row_bucket_of(2500, lv, cols, 40, 4, bits) for lv in range(bits // 8 - 1)]
    for u in rows:
        assert u.dtype == T.word_dtype(kind) and u.shape == (cols,)
        np.testing.assert_array_equal(T.u_of(T.raw_of(u, kind, largest), kind, largest), u)


@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("cols", [20001, 70001])
def test_narrow_level_of_the_generators(bits, cols):
    levels, cap = bits // 8, cols // 8
    for seed in (1, 2):
        for k in (1, 65, 1000, cols // 4):
            for lv in list(range(levels - 1)) + [T.NEVER]:
                u = T.row_narrowing_at(lv, cols, seed, bits)
                assert T.narrow_level(u, k, cap, levels) == lv, (bits, cols, seed, k, lv)
                np.testing.assert_array_equal(u, T.row_narrowing_at(lv, cols, seed, bits))  # deterministic
            kb = T.k_below_of(k)
            for lv in range(levels - 1):
                after = lv + 1 if lv + 1 < levels - 1 else T.NEVER  # where a bucket of cap + 1 narrows
                for size, want in ((cap, lv), (cap + 1, after), (1, lv), (cap // 2, lv)):
                    if not kb < k <= kb + size:
                        continue
                    u = T.row_bucket_of(size, lv, cols, kb, seed, bits)
                    shift = u.dtype.type(bits - 8 * (lv + 1))
                    kth = np.sort(u)[k - 1]
                    assert np.count_nonzero((u >> shift) == (kth >> shift)) == size
                    assert np.count_nonzero((u >> shift) < (kth >> shift)) == kb
                    assert T.narrow_level(u, k, cap, levels) == want, (bits, cols, seed, k, lv, size)


def test_narrow_level_plain_cases():
    u = np.arange(4096, dtype=np.uint32) << np.uint32(20)  # 16 keys per top byte
    assert T.narrow_level(u, 1, 16, 4) == 0
    assert T.narrow_level(u, 1, 15, 4) == 1  # one key per second digit
    assert T.narrow_level(np.full(100, 5, dtype=np.uint32), 7, 99, 4) is T.NEVER
    assert T.narrow_level(np.full(100, 5, dtype=np.uint32), 7, 100, 4) == 0
    assert T.narrow_level(np.full(100, 5, dtype=np.uint16), 7, 99, 2) is T.NEVER
    v = (np.arange(512, dtype=np.uint16) << np.uint16(7))  # two keys per top byte
    assert T.narrow_level(v, 300, 2, 2) == 0 and T.narrow_level(v, 300, 1, 2) is T.NEVER


def test_sweep_reaches_every_path_and_level(ls):
    """The cases of test_gpu_topk_select.py::test_seeded_sweep, planned on the host: both long-row
    paths, every narrowing level and every key type occur, and no row is short."""
    consts, tile = T.constants(), ls.segment_pair_tile_keys()
    paths, levels, kinds, edges = collections.Counter(), collections.Counter(), collections.Counter(), 0
    for seed in T.SWEEP_SEEDS:
        cases = list(T.sweep_cases(seed, tile, consts, ls.TOPK_SORT_DIV))
        assert len(cases) == T.SWEEP_CASES
        for c in cases:
            assert tile < c["cols"] <= 1 << 18 and c["rows"] * c["cols"] <= 1 << 20 and 1 <= c["k"] <= c["cols"]
            assert c["x"].shape == (c["rows"], c["cols"]) and c["x"].dtype == T.word_dtype(c["kind"])
            paths[c["path"]] += 1
            kinds[c["kind"]] += 1
            edges += abs(c["cols"] % consts["TK_CHUNK"] - consts["TK_CHUNK"] // 2) >= consts["TK_CHUNK"] // 2 - 1
            for lv in c["levels"] or ():
                levels[(T.bits_of(c["kind"]), lv)] += 1
    print("sweep paths (cases):", dict(paths), "short: 0")
    print("sweep narrowing levels (rows of select cases, by key width):", dict(levels))
    print("sweep key types:", dict(kinds), "chunk-edge widths:", edges)
    assert paths["select"] and paths["sort"] and set(kinds) == set(T.KINDS) and edges
    assert all(levels[(32, lv)] for lv in (0, 1, 2, T.NEVER)) and all(levels[(16, lv)] for lv in (0, T.NEVER))
