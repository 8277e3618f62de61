"""labsort_sort_pairs_device where only payloads can tell: run edges and ties, the AUTO boundary,
unaligned views and a seeded sweep.

A keys-only merge cannot show its tie rule (equal keys are identical words), so the rank, the cuts
and the level merges of the four-way pass, the pairwise pass and the tile sort are checked here
through the payload order, on the key/value kernels (k_m4_merge_kv, k_merge_pass_p<..., true>,
k_tile_sort<..., true>; tile: 16384 pairs).  The radix runs the same inputs through
k_onesweep_p<true>.  Protocol and expected result (the stable argsort of the order image):
tests/whole_sort_run.py, tests/whole_sort_model.py."""
import functools

import numpy as np
import pytest

import topk_model as T
import whole_sort_model as W
import whole_sort_run as R

pytestmark = pytest.mark.gpu

SEED = 0x9A125


@functools.lru_cache(maxsize=48)
def edge_case(shape, n, kind):
    """(words, perm) of one key shape, size and key type; shared by the two algorithms, never written."""
    x = W.shape_keys(shape, n, SEED, kind)
    perm = np.argsort(T.u_of(x, kind, False), kind="stable").astype(np.uint32)
    x.setflags(write=False)
    perm.setflags(write=False)
    return x, perm


# ---- run edges and ties ----

@pytest.mark.parametrize("m", list(range(1, 17)))
@pytest.mark.parametrize("algo", ["merge", "radix"])
def test_run_edges_with_payloads(ls, torch_gpu, algo, m):
    """n = m * 16384 + L for L in {1, 127, 128, 129}, the key/value counterpart of
    test_gpu_sort.py::test_merge_four_way_short_last_run.  merge: the last group of every four-way pass
    ends in a run of one pair, just under / exactly / just over one sample stride, at each of the four
    run positions as m varies, after a pairwise pass or not; radix: last tiles of 1, 127, 128 and 129
    pairs.  ties: five values, so every block cut falls inside runs of equal keys that span all four
    runs, and both key types' sentinel words are real keys of the last partial tile; const: the payloads
    come back as they went in; the sort of ties and its reverse; uniform.  Out of place with positions
    as payloads, in place with a bijection of them."""
    t = ls.pair_tile_keys()
    assert t == 16384
    failures, ncalls = [], 0
    for L in W.RUN_EDGE_TAILS:
        n = m * t + L
        for kind in ("u32", "i32"):
            for shape in W.PAIR_SHAPES:
                x, perm = edge_case(shape, n, kind)
                if shape == "const":
                    assert np.array_equal(perm, np.arange(n, dtype=np.uint32))
                for inplace in (False, True):
                    vals = W.payloads(n, bijection=inplace)
                    why = R.check_pairs(ls, torch_gpu, x, vals, x[perm], vals[perm], kind, algo, inplace)
                    ncalls += 1
                    if why:
                        failures.append(f"n={n} {kind} {shape} inplace={inplace}: {why} [{W.merge_shape(n, True)}]")
    assert not failures, f"{len(failures)} of {ncalls} calls: " + "; ".join(failures[:6])


# ---- the AUTO boundary ----

@pytest.mark.parametrize("side", ["at", "above"])
def test_auto_boundary(ls, torch_gpu, side):
    """LABSORT_ALGO_AUTO at LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS pairs (read from include/labsort.h) runs
    the merge sort, one pair more the radix: the result, and the launches the timing scopes count."""
    torch = torch_gpu
    bound = W.constants()["AUTO_PAIRS_MERGE_MAX_KEYS"]
    n = bound + (side == "above")
    x, perm = edge_case("ties", n, "i32")
    vals = W.payloads(n)
    ls.timing_enable(True)
    try:
        why = R.check_pairs(ls, torch, x, vals, x[perm], vals[perm], "i32", "auto", False)
        torch.cuda.synchronize()
        merge4, onesweep, tile = (ls.timing_read(c)[1] for c in ("merge4", "onesweep", "tile_sort"))
    finally:
        ls.timing_enable(False)
    assert why is None, why
    shape = W.merge_shape(n, True)
    if side == "at":
        assert onesweep == 0 and tile == 1 and merge4 == shape["passes"].count("four") >= 1, (merge4, onesweep, tile)
    else:
        assert (merge4, onesweep, tile) == (0, 4, 0)


# ---- unaligned views ----
# (keys, payloads) offsets in words: keys aligned and payloads not, keys not and payloads aligned, neither
OFFSET_COMBOS = [(0, 1), (3, 0), (1, 3)]


def view_calls():
    """(in place, offsets of keys in / payloads in / keys out / payloads out): each combination for the
    inputs (outputs aligned), for the outputs (inputs aligned) and for an in-place call."""
    calls = []
    for k, v in OFFSET_COMBOS:
        calls += [(False, (k, v, 0, 0)), (False, (0, 0, k, v)), (True, (k, v, k, v))]
    return calls


@pytest.mark.parametrize("shape", ["ties", "uniform", "const"])
@pytest.mark.parametrize("n", [100003, 300007])
@pytest.mark.parametrize("algo", ["radix", "merge"])
def test_pairs_unaligned_views(ls, torch_gpu, algo, n, shape):
    """Views that start 1 or 3 words into their buffers, between canaries.  include/labsort.h asks no
    alignment beyond the element's for this entry, so every call must succeed.  merge: one unaligned
    output pointer, the payloads' alone included, turns every four-way pass into a pairwise one
    (api.hip: `four`), whose 16-byte store test has a half for each output (k_merge_pass_p); radix:
    k_hist_seg's word path, the unaligned forms of pass 0's identity copy (const) and of the final
    copy (in place)."""
    kind = "i32" if shape == "ties" else "u32"
    x, perm = edge_case(shape, n, kind)
    failures = []
    for inplace, offs in view_calls():
        vals = W.payloads(n, bijection=inplace)
        why = R.check_pairs(ls, torch_gpu, x, vals, x[perm], vals[perm], kind, algo, inplace, offs)
        if why:
            failures.append(f"inplace={inplace} offs={offs}: {why}")
    assert not failures, f"{len(failures)} of {len(view_calls())} calls: " + "; ".join(failures)


@pytest.mark.parametrize("shape", ["uniform", "lowbyte", "const"])
def test_keys_unaligned_views_onesweep(ls, torch_gpu, monkeypatch, shape):
    """Keys only, the onesweep passes forced at the size of
    test_gpu_sort.py::test_sort_device_offsets_unaligned (which reaches the gathered passes and the
    merge only): out of place and in place.  lowbyte: one active pass, so the in-place call ends in the
    workspace and k_final_copy copies to an unaligned output; const: pass 0's identity copy."""
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    n = 200001
    assert ls.radix_impl(n) == "onesweep"
    x = W.shape_keys("uniform" if shape == "lowbyte" else shape, n, SEED + 1)
    if shape == "lowbyte":
        x = (x & np.uint32(0xFF)) | np.uint32(0x3C5A7100)
    failures = []
    for kind in ("u32", "i32"):
        ek, _ = W.expected(x, kind)
        for inplace, offs in [(False, (1, 3)), (False, (0, 1)), (False, (3, 0)), (True, (1, 1)), (True, (3, 3))]:
            why = R.check_keys(ls, torch_gpu, x, ek, kind, "radix", inplace, offs)
            if why:
                plan = W.radix_plan_model(T.u_of(x, kind, False), inplace)
                failures.append(f"{kind} inplace={inplace} offs={offs}: {why} [{W.plan_tag(plan)}]")
    assert not failures, "; ".join(failures)


# ---- the seeded sweep ----

@pytest.mark.parametrize("seed", W.PAIRS_SEEDS)
def test_seeded_sweep(ls, torch_gpu, seed):
    """The cases of whole_sort_model.pairs_sweep_cases: test_whole_sort_model.py asserts what the three
    seeds reach.  Every case runs; a failure names the case, its radix plan or merge shape."""
    failures, ncases = [], 0
    for c in W.pairs_sweep_cases(seed):
        n, kind = c["n"], c["kind"]
        vals = W.payloads(n, c["bijection"])
        ek, ev = W.expected(c["x"], kind, vals)
        why = R.check_pairs(ls, torch_gpu, c["x"], vals, ek, ev, kind, c["algo"], c["inplace"], c["offs"])
        ncases += 1
        if why:
            if c["runs"] == "radix":
                how = W.plan_tag(W.radix_plan_model(T.u_of(c["x"], kind, False), W.sorts_in_place(kind, c["inplace"])))
            else:
                how = str(W.merge_shape(n, True))
            failures.append(f"{c['tag']}: {why} [{how}]")
    assert ncases == W.PAIRS_CASES
    assert not failures, f"{len(failures)} of {ncases} cases: " + "; ".join(failures[:6])
