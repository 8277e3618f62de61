"""labsort_topk_device with float32 keys on the GPU: whole output arrays (keys and positions) against
the numpy model of the contract (tests/f32_model.py: the stable argsort of ord(key) ^ (largest ? ~0 : 0)),
on the three paths (rows sorted in LDS, the radix select, whole-row sorting) and across their
edges.  Keys compare NaN-ness everywhere and bit-exact otherwise, positions exactly.  Every call
runs on a workspace filled with 0xFF and outputs filled with a pattern, is followed by the status
call, and must leave its input as it was."""
import numpy as np
import pytest

import f32_model as M

pytestmark = pytest.mark.gpu

CHUNK = 16384  # the select's chunk (csrc/topk.h)
BOTH = [False, True]


def run(ls, torch, x, k, largest, ws=None, with_idx=True, key="f32"):
    rows, cols = x.shape
    d = torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()
    before = d.clone()
    ko = torch.full((rows, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    io = torch.full((rows, k), -7, dtype=torch.int32, device="cuda") if with_idx else None
    if ws is None:
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    # (float32 views of the same storage: what a caller with float data hands over)
    din, dout = (d.view(torch.float32), ko.view(torch.float32)) if key == "f32" else (d, ko)
    ls.topk_device(din, rows, cols, k, dout, io, largest=largest, key=key, workspace=ws)
    ls.topk_workspace_status(ws)
    assert torch.equal(d, before), "the input was written"
    return ko.cpu().numpy().view(np.uint32), (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, k, largest, **kw):
    ek, ei = M.topk_expected(x, k, largest)
    gk, gi = run(ls, torch, x, k, largest, **kw)
    msg = f"{x.shape} k={k} largest={largest}"
    M.assert_keys(gk, ek, msg)
    np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    return gk, gi


def with_ties(x, seed):
    """Every third column drawn from a few words: ties of ordinary values, NaNs and both zeros."""
    pool = np.array([0x3F800000, 0xBF800000, 0x7FC00000, 0xFFC00001, 0x80000000, 0x00000000, 0x7F800000], dtype=np.uint32)
    rng = np.random.default_rng(seed)
    x[:, ::3] = pool[rng.integers(0, pool.size, size=x[:, ::3].shape)]
    return x


def ks_long(ls, cols):
    d = ls.TOPK_SORT_DIV
    ks = {1, 2, 63, 64, 65, 1000, cols // d, cols // d + 1, cols // 2, cols - 1, cols}
    return sorted(k for k in ks if 1 <= k <= cols)


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (300, 257), (3, 4096), (2, 16384)])
def test_short_rows(ls, torch_gpu, rows, cols, largest):
    assert cols <= ls.segment_pair_tile_keys()
    x = with_ties(M.random_words((rows, cols), 0xF700 + rows), rows)
    if cols == 1:
        x[0, 0] = 0xFFC00001  # a lone NaN
    for k in sorted({1, min(2, cols), max(cols // 2, 1), cols}):
        check(ls, torch_gpu, x, k, largest)


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("dcols", [0, 1])
def test_short_long_edge(ls, torch_gpu, dcols, largest):
    cols = ls.segment_pair_tile_keys() + dcols
    x = M.random_words((3, cols), 0xF701)
    x[1] = M.tie_words((cols,), 0xF702)
    x[2, -40:] = 0x7FC00000  # NaNs in the last slots of a full tile
    for k in ks_long(ls, cols):
        check(ls, torch_gpu, x, k, largest)


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("rows,cols", [(1, 70001), (3, 70001), (5, 3 * CHUNK + 7)])
def test_long_rows(ls, torch_gpu, rows, cols, largest):
    assert cols > ls.segment_pair_tile_keys()
    x = M.random_words((rows, cols), 0xF703 + rows)
    x[rows - 1] = M.tie_words((cols,), 0xF704)  # one row of heavy ties beside the random ones
    if rows > 1:
        x[1] = M.normal_words((cols,), 0xF705)
    for k in ks_long(ls, cols):
        check(ls, torch_gpu, x, k, largest)


DCOLS = 200003  # odd (row 1 starts unaligned), 13 chunks
NEG0, POS0 = 0x80000000, 0x00000000


def dist_rows(name):
    rng = np.random.default_rng(0xF706)
    n = DCOLS
    if name == "normal":
        return M.normal_words((2, n), 1)
    if name == "all_nan":      # never narrows; positions must come out 0 .. k-1
        x = np.full((2, n), 0x7FC00000, dtype=np.uint32)
        x[:, 1::2] = 0xFFC00001
        x[:, 2::7] = 0x7F800001
        return x
    if name == "neg_zero":
        return np.full((2, n), NEG0, dtype=np.uint32)
    if name == "zeros":        # half -0.0, half +0.0
        return np.where(rng.random((2, n)) < 0.5, np.uint32(NEG0), np.uint32(POS0)).astype(np.uint32)
    if name in ("infs", "infs_rev"):  # 6 % of one infinity, 92 % of the other, the rest random
        lo, hi = (0xFF800000, 0x7F800000) if name == "infs" else (0x7F800000, 0xFF800000)
        x = M.random_words((2, n), 5)
        r = rng.random((2, n))
        x[r < 0.06] = lo
        x[r > 0.08] = hi
        return x
    if name == "mantissa":     # one sign and exponent, random mantissas: narrows only at level 2
        return (M.random_words((2, n), 7, plant=False) & np.uint32(0x0000FFFF)) | np.uint32(0x40490000)
    raise ValueError(name)


@pytest.mark.parametrize("name", ["normal", "all_nan", "neg_zero", "zeros", "infs", "infs_rev", "mantissa"])
def test_distributions(ls, torch_gpu, name):
    x = dist_rows(name)
    ks = (1, 1000, 20000, DCOLS // ls.TOPK_SORT_DIV)
    assert max(ks) * ls.TOPK_SORT_DIV <= DCOLS  # the select runs
    for largest in BOTH:
        for k in ks:
            gk, gi = check(ls, torch_gpu, x, k, largest)
            if name in ("all_nan", "neg_zero"):
                np.testing.assert_array_equal(gi, np.tile(np.arange(k, dtype=np.uint32), (2, 1)))
            if name == "zeros":  # every -0.0 first when ascending, last when descending
                want = NEG0 if not largest else POS0
                nfirst = np.minimum((x == want).sum(axis=1), k)
                for r in range(2):
                    assert np.all(gk[r, :nfirst[r]] == want) and np.all(gk[r, nfirst[r]:] == (want ^ NEG0))


def test_nan_ties_at_the_threshold(ls, torch_gpu):
    """30 % NaN: with largest the NaNs come first, so the k-th key is a NaN and the NaN ties taken are
    those with the lowest positions; a run of NaNs lies across a chunk boundary and k cuts inside it."""
    rng = np.random.default_rng(0xF707)
    x = M.random_words((2, DCOLS), 8)
    r = rng.random((2, DCOLS))
    x[r < 0.15] = 0x7FC00000
    x[(r >= 0.15) & (r < 0.30)] = 0xFFC00001
    bounds = (CHUNK, 2 * CHUNK)
    for row, b in enumerate(bounds):
        x[row, b - 5:b + 6] = 0x7F800001  # 11 NaN ties around the boundary
    nan = M.is_nan(x)
    # k = NaNs before the run + 6: the last one taken is the first word past the boundary (row 0)
    k_cut = int(nan[0, :CHUNK - 5].sum()) + 6
    assert k_cut * ls.TOPK_SORT_DIV <= DCOLS
    for k in (1, 1000, k_cut, 20000, DCOLS // ls.TOPK_SORT_DIV):
        gk, gi = check(ls, torch_gpu, x, k, True)
        assert np.all(M.is_nan(gk))
        for row in range(2):
            np.testing.assert_array_equal(gi[row], np.flatnonzero(nan[row])[:k])
    _, gi = run(ls, torch_gpu, x, k_cut, True)
    assert list(gi[0, -6:]) == list(range(CHUNK - 5, CHUNK + 1))
    # ascending, k past the non-NaN count: the tail of the output is the first NaNs (whole-row sort path)
    k = int((~nan[0]).sum()) + 10
    gk, gi = check(ls, torch_gpu, x[:1], k, False)
    np.testing.assert_array_equal(gi[0, -10:], np.flatnonzero(nan[0])[:10])


@pytest.mark.parametrize("rows,cols,k", [(300, 257, 9), (3, 70001, 65), (1, 70001, 40000)])
def test_without_indices(ls, torch_gpu, rows, cols, k):
    x = with_ties(M.random_words((rows, cols), 0xF708), 3)
    gk, _ = run(ls, torch_gpu, x, k, True)
    nk, none = run(ls, torch_gpu, x, k, True, with_idx=False)
    assert none is None
    M.assert_keys(nk, gk)
    M.assert_keys(nk, M.topk_expected(x, k, True)[0])


def test_workspace_reused_across_key_types(ls, torch_gpu):
    torch = torch_gpu
    calls = [((3, 70001), 1000, "f32", False), ((2, 50000), 77, "i32", True), ((40, 300), 300, "f32", True),
             ((1, 70001), 60000, "u32", True), ((3, 70001), 1000, "f32", True), ((2, 40000), 9, "u32", False),
             ((1, 70001), 60000, "f32", False)]
    size = max(ls.topk_workspace_bytes(s[0], s[1], k) for s, k, *_ in calls)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (shape, k, key, largest) in enumerate(calls):
        x = M.tie_words(shape, 0xF709 + i) if i % 2 else M.random_words(shape, 0xF709 + i)
        if key == "f32":
            check(ls, torch, x, k, largest, ws=ws)
            continue
        u = x ^ np.uint32((0x80000000 if key == "i32" else 0) ^ (0xFFFFFFFF if largest else 0))
        idx = np.argsort(u, axis=1, kind="stable")[:, :k]
        gk, gi = run(ls, torch, x, k, largest, ws=ws, key=key)
        np.testing.assert_array_equal(gk, np.take_along_axis(x, idx, axis=1))
        np.testing.assert_array_equal(gi, idx.astype(np.uint32))


@pytest.mark.parametrize("rows,cols,k", [(2, 100003, 500), (4, 3000, 10)])
def test_graph_replay(ls, torch_gpu, rows, cols, k):
    """One captured call replayed on new keys in the same buffers."""
    torch = torch_gpu
    src = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    ko = torch.zeros((rows, k), dtype=torch.float32, device="cuda")
    io = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.topk_device(src, rows, cols, k, ko, io, largest=True, key="f32", workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.topk_device(src, rows, cols, k, ko, io, largest=True, key="f32", workspace=ws, stream=torch.cuda.current_stream())
    inputs = {"normal": M.normal_words((rows, cols), 0xF70A),
              "all_nan": np.full((rows, cols), 0xFFC00001, dtype=np.uint32),
              "const": np.full((rows, cols), 0xC0490FDB, dtype=np.uint32),
              "random_bits": M.random_words((rows, cols), 0xF70B)}
    for dist, x in inputs.items():
        src.view(torch.int32).copy_(torch.from_numpy(x.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.topk_workspace_status(ws)
        ek, ei = M.topk_expected(x, k, True)
        M.assert_keys(ko.view(torch.int32).cpu().numpy().view(np.uint32), ek, dist)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=dist)


@pytest.mark.parametrize("shape,k,kind", [((300, 257), 128, "ties"), ((3, 70001), 1000, "random"), ((2, DCOLS), 20000, "normal")])
def test_values_match_torch_topk(ls, torch_gpu, shape, k, kind):
    """Values only (torch leaves the tie order open), NaN-equal ==, against torch.topk on the CPU tensor."""
    torch = torch_gpu
    x = {"ties": M.tie_words, "random": M.random_words, "normal": M.normal_words}[kind](shape, 0xF70C)
    t = torch.from_numpy(x.view(np.float32).copy())
    for largest in BOTH:
        gk, _ = run(ls, torch, x, k, largest)
        want = torch.topk(t, k, dim=1, largest=largest, sorted=True).values.numpy()
        got = gk.view(np.float32)
        assert np.all((got == want) | (np.isnan(got) & np.isnan(want))), (shape, k, largest)
