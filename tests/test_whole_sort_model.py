"""tests/whole_sort_model.py on the host: the digit-mask arrays hold exactly the mask they were asked
for at every size the GPU tests use, the sixteen masks reach every branch of the radix plan the
GPU tests are meant to run, the model's constants are the library's, and the three seeds of the
key/value sweep reach every algorithm, plan shape, merge shape and view combination.  Nothing here
launches a kernel."""
import numpy as np
import pytest

import sort_sweep_model as S
import topk_model as T
import whole_sort_model as W

BOTH = [False, True]
MASK_SIZES = sorted(set(W.ONESWEEP_SIZES + W.PAIR_TILE_SIZES + (W.GATHER_FUSED_SIZE,)))


def test_constants_are_the_librarys(ls):
    c = W.constants()
    assert c["TILE_KEYS"] == ls.tile_keys() == 32768 and c["PAIR_TILE"] == ls.pair_tile_keys() == 16384
    assert c["MG_TILE"] == ls.merge_tile_keys() and c["OSP_TILE"] == 16384 and c["OSP_LBW"] == 8 and c["NSEG"] == 16
    # key/value: radix and merge workspaces differ on the two sides of the AUTO bound
    a = c["AUTO_PAIRS_MERGE_MAX_KEYS"]
    assert ls.pairs_workspace_bytes(a, "auto") == ls.pairs_workspace_bytes(a, "merge")
    assert ls.pairs_workspace_bytes(a + 1, "auto") == ls.pairs_workspace_bytes(a + 1, "radix")
    # the sizes of test_gpu_whole_masks.py are where its docstring says
    lo, hi = W.ONESWEEP_SIZES
    assert c["TILE_KEYS"] < lo and -(-lo // c["OSP_TILE"]) == 3 and lo // c["NSEG"] < c["OSP_TILE"]
    assert -(-hi // c["OSP_TILE"]) == 19 > 2 * c["OSP_LBW"]  # one chain looks back over three windows
    groups = lambda n: -(-(-(-n // c["GS_TILE"])) // c["GS_GROUP"])  # noqa: E731
    assert groups(W.GATHER_FUSED_SIZE) == 1 <= c["GS_SMALL_NG"] < groups(W.GATHER_SIZE) == c["GS_SMALL_NG"] + 1
    assert groups(1 << 20) == c["GS_SMALL_NG"]  # (the last fused size)
    assert all(n <= c["PAIR_TILE"] for n in W.PAIR_TILE_SIZES)


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("n", MASK_SIZES)
def test_mask_arrays_hold_their_mask(kind, n):
    arrays = W.mask_arrays(kind, n, W.MASK_SEED)
    assert len(arrays) == 80 and {v for (_, v), _ in arrays} == set(S.VARIANTS)
    for (m, v), x in arrays:
        assert x.shape == (n,) and x.dtype == np.uint32
        u = T.u_of(x, kind, False)
        assert S.mask_of(u[None])[0] == m, (kind, n, m, v)
        # the model's active digits are the mask's
        assert W.radix_plan_model(u, False)["active"] == [p for p in range(4) if (m >> p) & 1], (kind, n, m, v)
    if kind != "f32":
        for (m, v), x in W.ff_arrays(kind, n, W.MASK_SEED):
            u = T.u_of(x, kind, False)
            assert S.mask_of(u[None])[0] == m
            for p in range(4):
                if not (m >> p) & 1:
                    assert bool((((u >> np.uint32(8 * p)) & np.uint32(0xFF)) == 0xFF).all())


@pytest.mark.parametrize("kind", ["u32", "i32"])
def test_gather_size_mask_arrays(kind):
    arrays = W.mask_arrays(kind, W.GATHER_SIZE, W.MASK_SEED, W.GATHER_VARIANTS)
    assert len(arrays) == 48
    for (m, v), x in arrays:
        assert S.mask_of(T.u_of(x, kind, False)[None])[0] == m, (m, v)


def test_plan_model_reach_of_the_masks():
    """Both in_place values with 0 .. 4 active passes, the keys in OUT after every out-of-place plan
    with a pass, both first-pass modes, both later-pass modes, the three copy_from values."""
    n = 1000
    arrays = W.mask_arrays("u32", n, W.MASK_SEED, ("full",))
    first, later, copies = set(), set(), set()
    for in_place in BOTH:
        counts = set()
        for (m, _), x in arrays:
            p = W.radix_plan_model(T.u_of(x, "u32", False), in_place)
            k = len(p["active"])
            counts.add(k)
            assert k == bin(m).count("1") == len(p["route"]) == len(p["modes"])
            copies.add(p["copy_from"])
            for i, (src, dst) in enumerate(p["route"]):
                assert src != dst and src == (W.IN if i == 0 else p["route"][i - 1][1])  # no pass scatters in place
                assert (src, dst) != (W.IN, W.OUT) or not in_place
            if k:
                first.add(p["modes"][0])
                later.update(p["modes"][1:])
                last = p["route"][-1][1]
                if not in_place:
                    assert last == W.OUT and p["copy_from"] == W.SKIP, (m, p)
                else:  # IN is OUT: an odd count of passes ends in TMP and is copied from there
                    assert (last, p["copy_from"]) == ((W.TMP, W.TMP) if k & 1 else (W.OUT, W.SKIP)), (m, p)
            else:
                assert p["copy_from"] == (W.SKIP if in_place else W.IN)
        assert counts == {0, 1, 2, 3, 4}
    assert first == {0, 2} and later == {1, 2} and copies == {W.SKIP, W.IN, W.TMP}
    # the rule's edge: one key that differs makes the digit active, a count of n - 1 is not trivial
    u = np.full(n, 0x11223344, dtype=np.uint32)
    assert W.radix_plan_model(u, False)["active"] == []
    u[n // 2] ^= np.uint32(0x00010000)
    assert W.radix_plan_model(u, False)["active"] == [2]
    assert W.sorts_in_place("f32", False) and not W.sorts_in_place("i32", False) and W.sorts_in_place("u32", True)


def test_long_nibble_segments_and_segments_of_one_key():
    """At the larger onesweep size the onebit and lone_* arrays put at least 9 tiles into one segment
    of every pass that runs in mode 1 (more than one look-back window), and lone_* arrays make
    segments of exactly one key."""
    c = W.constants()
    n = W.ONESWEEP_SIZES[1]
    need = (c["OSP_LBW"] + 1) * c["OSP_TILE"]
    one_key = {v: 0 for v in S.VARIANTS if v.startswith("lone")}
    mode1 = 0
    for (m, v), x in W.mask_arrays("u32", n, W.MASK_SEED, ("onebit", "lone_first", "lone_last", "lone_mid")):
        u = T.u_of(x, "u32", False)
        p = W.radix_plan_model(u, False)
        for q, mode in zip(p["active"], p["modes"]):
            if mode == 1:
                mode1 += 1
                seg = W.nibble_segments(u, q)
                assert int(seg.sum()) == n and int(seg.max()) >= need, (m, v, q, seg)
                if v in one_key and int(seg.min(initial=n, where=seg > 0)) == 1:
                    one_key[v] += 1
    assert mode1 >= 4 * 11  # (the masks with two neighbouring digits)
    assert all(k >= 4 for k in one_key.values()), one_key


def test_merge_shape():
    c = W.constants()
    t = c["PAIR_TILE"]
    assert W.merge_shape(t, True)["levels"] == 0 and W.merge_shape(t + 1, True)["passes"] == ["pair"]
    # tests/test_gpu_sort.py::test_driver_launch_structure, as counted on the device
    assert W.merge_shape(1 << 20, False)["passes"] == ["pair", "four", "four"]
    assert W.merge_shape((1 << 20) + 1, False)["passes"] == ["four", "four", "four"]
    assert W.merge_shape(1 << 20, True)["passes"] == ["four", "four", "four"]
    assert W.merge_shape((1 << 20) + 1, True)["passes"] == ["pair", "four", "four", "four"]
    s = W.merge_shape(5 * t + 129, True)  # 6 runs, 3 levels: a pairwise pass, then runs of 2 t
    assert s["levels"] == 3 and s["fours"] == [dict(r=2 * t, last_group_runs=3, last_run=t + 129)]
    # the run-edge sizes of test_gpu_pairs.py: every count of runs in the last group, with each tail
    seen = set()
    for m in range(1, 17):
        for L in W.RUN_EDGE_TAILS:
            for f in W.merge_shape(m * t + L, True)["fours"]:
                seen.add((f["last_group_runs"], f["last_run"] % t if f["last_run"] % t in W.RUN_EDGE_TAILS else 0))
    assert {a for a, _ in seen} == {1, 2, 3, 4} and {b for _, b in seen} >= set(W.RUN_EDGE_TAILS)


def test_shape_keys():
    for kind in ("u32", "i32"):
        x = W.shape_keys("ties", 5000, 1, kind)
        assert set(np.unique(x)) == set(W.TIE_VALUES)
        u = T.u_of(W.shape_keys("sorted_ties", 5000, 1, kind), kind).astype(np.int64)
        assert bool((np.diff(u) >= 0).all()) and np.unique(u).size == 5
        u = T.u_of(W.shape_keys("reversed_ties", 5000, 1, kind), kind).astype(np.int64)
        assert bool((np.diff(u) <= 0).all()) and np.unique(u).size == 5
    assert np.unique(W.shape_keys("const", 100, 2)).size == 1
    # the sentinel words (~flip) of both key types are among the tie values
    assert 0xFFFFFFFF in W.TIE_VALUES and 0x7FFFFFFF in W.TIE_VALUES
    v = W.payloads(1 << 16, True)
    assert np.unique(v).size == v.size and not np.array_equal(v, W.payloads(1 << 16))


def test_pairs_sweep_coverage():
    c = W.constants()
    t, auto = c["PAIR_TILE"], c["AUTO_PAIRS_MERGE_MAX_KEYS"]
    cases = [k for seed in W.PAIRS_SEEDS for k in W.pairs_sweep_cases(seed, c)]
    assert len(cases) == len(W.PAIRS_SEEDS) * W.PAIRS_CASES and 60 <= W.PAIRS_CASES <= 80
    assert len({k["tag"] for k in cases}) == len(cases)
    assert sum(k["n"] for k in cases) < 60_000_000  # (the reference: about 0.1 s per million keys)
    edges = set(W.sweep_edge_sizes(c))
    assert {1, 2, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, auto, auto + 1, (1 << 20) - 1, (1 << 20) + 1} <= edges
    assert sum(k["n"] in edges for k in cases) >= len(cases) // 3
    masks, first, later, counts, levels, groups = set(), set(), set(), set(), set(), set()
    for k in cases:
        assert k["x"].shape == (k["n"],) and k["x"].dtype == np.uint32 and 1 <= k["n"] <= 1 << 21
        assert not k["inplace"] or k["offs"][:2] == k["offs"][2:]
        u = T.u_of(k["x"], k["kind"], False)
        if k["gen"].startswith("mask:") and k["n"] > 1:
            assert S.mask_of(u[None])[0] == int(k["gen"].split(":")[1]), k["tag"]
        if k["runs"] == "radix":
            p = W.radix_plan_model(u, W.sorts_in_place(k["kind"], k["inplace"]))
            counts.add(len(p["active"]))
            first.update(p["modes"][:1])
            later.update(p["modes"][1:])
            if k["gen"].startswith("mask:"):
                masks.add(int(k["gen"].split(":")[1]))
        if k["runs"] == "merge":
            s = W.merge_shape(k["n"], True, c)
            levels.add(s["levels"])
            groups.update(f["last_group_runs"] for f in s["fours"])
    assert {(k["algo"], k["inplace"]) for k in cases} == {(a, b) for a in W.ALGOS for b in BOTH}
    assert masks == set(range(16)), masks
    assert first == {0, 2} and later == {1, 2} and counts == {0, 1, 2, 3, 4}
    assert levels == {1, 2, 3, 4, 5, 6, 7}, levels
    assert groups == {1, 2, 3, 4}
    assert any(k["runs"] == "tile" for k in cases)
    assert {k["runs"] for k in cases if k["algo"] == "auto" and k["n"] > t} == {"merge", "radix"}
    assert any(k["algo"] == "auto" and t < k["n"] <= auto for k in cases) and any(k["algo"] == "auto" and k["n"] > auto for k in cases)
    assert {k["kind"] for k in cases} == set(W.KINDS)
    assert {k["gen"] for k in cases if not k["gen"].startswith("mask:")} == set(W.PLAIN_GENS)
    assert {k["gen"].split(":")[2] for k in cases if k["gen"].startswith("mask:")} == set(S.VARIANTS)
    # a call whose only unaligned pointer is a payload pointer, under the merge sort (api.hip:
    # "four" turns every four-way pass into a pairwise one) and under the radix
    only_payload = [k for k in cases if k["n"] > t and k["offs"][0] == k["offs"][2] == 0 and (k["offs"][1] or k["offs"][3])]
    assert {k["runs"] for k in only_payload} == {"merge", "radix"}, [k["tag"] for k in only_payload]
    assert any(any(k["offs"]) for k in cases if k["inplace"]) and any(not any(k["offs"]) for k in cases)
