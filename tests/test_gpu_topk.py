"""labsort_topk_device on the GPU: whole output arrays (keys and positions) against numpy's stable
argsort of u = key ^ flip ^ (largest ? ~0 : 0), on every path (rows sorted in LDS, the radix
select, whole-row sorting above the large-k threshold) and on both sides of the edges between
them.  Every call runs on a workspace filled with 0xFF and outputs filled with a pattern, is
followed by the status call, and must leave its input as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMBOS = [("u32", False), ("u32", True), ("i32", False), ("i32", True)]
CHUNK = 16384  # the select's chunk (csrc/topk.h)


def expected(x, k, key, largest):
    """x: (rows, cols) uint32 words.  The first k of each row's stable sort on u."""
    u = x ^ np.uint32((0x80000000 if key == "i32" else 0) ^ (0xFFFFFFFF if largest else 0))
    idx = np.argsort(u, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def run(ls, torch, x, k, key, largest, ws=None, with_idx=True, d=None):
    rows, cols = x.shape
    if d is None:
        d = torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()
    before = d.clone()
    ko = torch.full((rows, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    io = torch.full((rows, k), -7, dtype=torch.int32, device="cuda") if with_idx else None
    if ws is None:
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.topk_device(d, rows, cols, k, ko, io, largest=largest, key=key, workspace=ws)
    ls.topk_workspace_status(ws)
    assert torch.equal(d, before), "the input was written"
    return ko.cpu().numpy().view(np.uint32), (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, k, key, largest, **kw):
    ek, ei = expected(x, k, key, largest)
    gk, gi = run(ls, torch, x, k, key, largest, **kw)
    np.testing.assert_array_equal(gk, ek, err_msg=f"keys {x.shape} k={k} {key} largest={largest}")
    np.testing.assert_array_equal(gi, ei, err_msg=f"positions {x.shape} k={k} {key} largest={largest}")


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def ks_of(ls, cols, extra=()):
    d = ls.TOPK_SORT_DIV
    ks = {1, 2, cols // 2, cols, cols // d, cols // d + 1, cols - 1, *extra}
    return sorted(k for k in ks if 1 <= k <= cols)


@pytest.mark.parametrize("key,largest", COMBOS)
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (300, 257), (3, 4096), (2, 16384)])
def test_short_rows(ls, torch_gpu, rows, cols, key, largest):
    assert cols <= ls.segment_pair_tile_keys()
    x = rand((rows, cols), 0x70C0 + rows)
    x[:, ::3] %= 50  # ties, and small values among the random ones
    for k in sorted({1, min(2, cols), max(cols // 2, 1), cols}):
        check(ls, torch_gpu, x, k, key, largest)


@pytest.mark.parametrize("key,largest", COMBOS)
@pytest.mark.parametrize("dcols", [0, 1])
def test_short_long_edge(ls, torch_gpu, dcols, key, largest):
    cols = ls.segment_pair_tile_keys() + dcols
    x = rand((3, cols), 0x70C1)
    x[1] %= 100
    for k in ks_of(ls, cols, (64,)):
        check(ls, torch_gpu, x, k, key, largest)


@pytest.mark.parametrize("key,largest", COMBOS)
@pytest.mark.parametrize("rows,cols", [(1, 70001), (3, 70001), (5, 3 * CHUNK + 7)])
def test_long_rows(ls, torch_gpu, rows, cols, key, largest):
    assert cols > ls.segment_pair_tile_keys()
    x = rand((rows, cols), 0x70C2 + rows)
    x[rows - 1] %= 1000  # one row of heavy ties beside the random ones
    for k in ks_of(ls, cols, (63, 64, 65, 1000)):
        check(ls, torch_gpu, x, k, key, largest)


DCOLS = 200003  # odd (row 1 starts unaligned), 13 chunks, k = 20000 below cols // 8


def dist_rows(name):
    rng = np.random.default_rng(0x70C3)
    n = DCOLS
    if name == "uniform":      # narrows after level 0
        return rand((2, n), 1)
    if name == "const":        # never narrows; positions must come out 0 .. k-1
        return np.full((2, n), 0xDEADBEEF, dtype=np.uint32)
    if name == "mod100":       # three trivial digits, huge ties, never narrows
        return rand((2, n), 2) % np.uint32(100)
    if name == "sorted":
        return np.sort(rand((2, n), 3), axis=1)
    if name == "reversed":
        return np.sort(rand((2, n), 4), axis=1)[:, ::-1].copy()
    if name == "extremes":     # 0 and 0xFFFFFFFF many times; the threshold falls on either
        x = rand((2, n), 5)
        r = rng.random((2, n))
        x[r < 0.06] = 0
        x[r > 0.08] = 0xFFFFFFFF
        return x
    if name == "extremes_rev":  # the same with the masses swapped
        x = rand((2, n), 6)
        r = rng.random((2, n))
        x[r < 0.06] = 0xFFFFFFFF
        x[r > 0.08] = 0
        return x
    if name == "top16":        # random keys sharing their top 16 bits: narrows only at level 2
        return (rand((2, n), 7) & np.uint32(0xFFFF)) | np.uint32(0x7FFE0000)
    if name == "straddle":     # the k-th key's ties lie on both sides of a chunk boundary
        x = rand((2, n), 8) | np.uint32(0x40000000)
        for r, b in ((0, CHUNK), (1, 2 * CHUNK)):
            x[r, 100:200] = np.arange(100, dtype=np.uint32)      # 100 keys below the tie value
            x[r, b - 5:b + 6] = 1000                              # 11 ties around the boundary
        return x
    raise ValueError(name)


@pytest.mark.parametrize("name", ["uniform", "const", "mod100", "sorted", "reversed", "extremes", "extremes_rev",
                                  "top16", "straddle"])
def test_distributions(ls, torch_gpu, name):
    x = dist_rows(name)
    ks = (106,) if name == "straddle" else (1, 1000, 20000, DCOLS // ls.TOPK_SORT_DIV)
    assert all(k % CHUNK for k in ks) and max(ks) * ls.TOPK_SORT_DIV <= DCOLS  # the select runs
    for key, largest in (COMBOS if name.startswith("extremes") else [("u32", False), ("i32", True)]):
        if name == "straddle" and largest:
            continue
        for k in ks:
            check(ls, torch_gpu, x, k, key, largest)
    if name == "const":
        _, gi = run(ls, torch_gpu, x, 20000, "u32", False)
        np.testing.assert_array_equal(gi, np.tile(np.arange(20000, dtype=np.uint32), (2, 1)))
    if name == "straddle":  # the six ties taken are the first six, across the boundary
        _, gi = run(ls, torch_gpu, x, 106, "u32", False)
        assert list(gi[0, 100:]) == list(range(CHUNK - 5, CHUNK + 1))
        assert list(gi[1, 100:]) == list(range(2 * CHUNK - 5, 2 * CHUNK + 1))


@pytest.mark.parametrize("dist", ["uniform", "mod1000"])
def test_mid_size(ls, torch_gpu, dist):
    n = 1 << 22
    x = rand((1, n), 0x70C4)
    if dist == "mod1000":
        x %= np.uint32(1000)
    check(ls, torch_gpu, x, 1000, "i32", dist == "uniform")


@pytest.mark.parametrize("rows,cols,k", [(300, 257, 9), (3, 70001, 65), (1, 70001, 40000)])
def test_without_indices(ls, torch_gpu, rows, cols, k):
    x = rand((rows, cols), 0x70C5) % np.uint32(5000)
    gk, _ = run(ls, torch_gpu, x, k, "u32", True)
    nk, none = run(ls, torch_gpu, x, k, "u32", True, with_idx=False)
    assert none is None
    np.testing.assert_array_equal(nk, gk)
    np.testing.assert_array_equal(nk, expected(x, k, "u32", True)[0])


def test_workspace_reused(ls, torch_gpu):
    torch = torch_gpu
    calls = [((3, 70001), 1000, "u32", False, "uniform"), ((2, 50000), 77, "i32", True, "mod"),
             ((40, 300), 300, "i32", False, "uniform"), ((1, 70001), 60000, "u32", True, "mod"),
             ((3, 70001), 1000, "u32", False, "mod")]
    size = max(ls.topk_workspace_bytes(s[0], s[1], k) for s, k, *_ in calls)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (shape, k, key, largest, dist) in enumerate(calls):
        x = rand(shape, 0x70C6 + i)
        if dist == "mod":
            x %= np.uint32(100)
        check(ls, torch, x, k, key, largest, ws=ws)


@pytest.mark.parametrize("rows,cols,k", [(2, 100003, 500), (1, 100003, 500), (4, 3000, 10)])
def test_graph_replay(ls, torch_gpu, rows, cols, k):
    """One captured call replayed on new keys in the same buffers: a distribution that narrows
    (uniform) and ones that do not (% 100, constant)."""
    torch = torch_gpu
    src = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ko = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    io = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.topk_device(src, rows, cols, k, ko, io, key="i32", workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.topk_device(src, rows, cols, k, ko, io, key="i32", workspace=ws, stream=torch.cuda.current_stream())
    for i, dist in enumerate(("uniform", "mod100", "uniform", "const")):
        x = rand((rows, cols), 0x70C7 + i)
        if dist == "mod100":
            x %= np.uint32(100)
        if dist == "const":
            x[:] = 0x80000001
        src.copy_(torch.from_numpy(x.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.topk_workspace_status(ws)
        ek, ei = expected(x, k, "i32", False)
        np.testing.assert_array_equal(ko.cpu().numpy().view(np.uint32), ek, err_msg=dist)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=dist)
