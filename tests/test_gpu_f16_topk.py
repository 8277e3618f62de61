"""labsort_topk_device with bfloat16 / float16 keys on the GPU: whole output arrays (keys and
positions) against the numpy model of the contract (tests/f16_model.py: the stable argsort of
ord16(key) ^ (largest ? 0xFFFF : 0)), on the three paths (rows sorted in LDS, the radix select,
whole-row sorting) and across their edges.  Keys compare NaN-ness everywhere and bit-exact
otherwise, positions exactly.  Every call runs on a workspace filled with 0xFF and outputs filled
with a pattern, is followed by the status call, and must leave its input as it was.  With 65536
possible values every long row is full of ties, so the tie order at the threshold is exercised
throughout."""
import numpy as np
import pytest

import f16_model as M
import f32_model as F

pytestmark = pytest.mark.gpu

CHUNK = 16384  # the select's chunk (csrc/topk.h)
BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", M.KINDS)


def tdtype(torch, kind):
    return torch.bfloat16 if kind == "bf16" else torch.float16


def run(ls, torch, x, k, largest, kind, ws=None, with_idx=True, in_off=0, out_off=0):
    """in_off / out_off: elements between the start of the storage and the matrix (1: a base
    address that is 2-byte but not 4-byte aligned)."""
    rows, cols = x.shape
    store = torch.full((rows * cols + in_off,), 0x1111, dtype=torch.int16, device="cuda")
    d = store[in_off:].view(rows, cols)
    d.copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.int16)))
    before = store.clone()
    ostore = torch.full((rows * k + out_off + 1,), 0x5A5A, dtype=torch.int16, device="cuda")
    ko = ostore[out_off:out_off + rows * k].view(rows, k)
    io = torch.full((rows, k), -7, dtype=torch.int32, device="cuda") if with_idx else None
    if ws is None:
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    assert d.is_contiguous() and ko.is_contiguous() and d.data_ptr() % 4 == 2 * (in_off % 2)
    # (views of the type over the same storage: what a caller with 16-bit float data hands over)
    ls.topk_device(d.view(tdtype(torch, kind)), rows, cols, k, ko.view(tdtype(torch, kind)), io, largest=largest, key=kind,
                   workspace=ws)
    ls.topk_workspace_status(ws)
    assert torch.equal(store, before), "the input was written"
    assert int(ostore[-1]) == 0x5A5A and (out_off == 0 or int(ostore[0]) == 0x5A5A), "written outside the output"
    return ko.cpu().numpy().view(np.uint16), (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, k, largest, kind, **kw):
    ek, ei = M.topk_expected(x, k, largest, kind)
    gk, gi = run(ls, torch, x, k, largest, kind, **kw)
    msg = f"{kind} {x.shape} k={k} largest={largest}"
    M.assert_keys(gk, ek, kind, msg)
    np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    return gk, gi


def ks_long(ls, cols):
    d = ls.TOPK_SORT_DIV
    ks = {1, 2, 63, 64, 65, 1000, cols // d, cols // d + 1, cols // 2, cols - 1, cols}
    return sorted(k for k in ks if 1 <= k <= cols)


@KINDS
@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 5), (300, 257), (2, 16384)])
def test_short_rows(ls, torch_gpu, rows, cols, largest, kind):
    assert cols <= ls.segment_pair_tile_keys()
    x = M.random_words((rows, cols), 0xF160 + rows, kind)
    x[:, ::3] = M.tie_words((rows, cols), rows, kind)[:, ::3]
    if cols == 1:
        x[0, 0] = M.specials(kind)["-qnan1"]  # a lone NaN
    for k in sorted({1, min(2, cols), max(cols // 2, 1), cols}):
        check(ls, torch_gpu, x, k, largest, kind)


@KINDS
@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("dcols", [0, 1])
def test_short_long_edge(ls, torch_gpu, dcols, largest, kind):
    cols = ls.segment_pair_tile_keys() + dcols
    x = M.random_words((3, cols), 0xF161, kind)
    x[1] = M.tie_words((cols,), 0xF162, kind)
    x[2, -40:] = M.specials(kind)["qnan"]  # NaNs in the last slots of a full tile
    for k in sorted({1, 64, 65, cols // 4, cols // 4 + 1, cols - 1, cols}):
        check(ls, torch_gpu, x, k, largest, kind)


@KINDS
@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("rows,cols", [(8, 70001), (5, 3 * CHUNK + 7)])
def test_long_rows(ls, torch_gpu, rows, cols, largest, kind):
    """(8, 70001): row r starts r mod 8 elements into a 16-byte line, so all eight misalignments of
    the 16-byte loads occur."""
    assert cols > ls.segment_pair_tile_keys()
    if rows == 8:
        assert sorted((r * cols) % 8 for r in range(rows)) == list(range(8))
    x = M.random_words((rows, cols), 0xF163 + rows, kind)
    x[rows - 1] = M.tie_words((cols,), 0xF164, kind)  # one row of heavy ties beside the random ones
    x[1] = M.normal_words((cols,), 0xF165, kind)
    for k in ks_long(ls, cols):
        check(ls, torch_gpu, x, k, largest, kind)


@KINDS
@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1)])
def test_odd_base_address(ls, torch_gpu, in_off, out_off, kind):
    """The matrix starts one element into its storage: 2-byte but not 4-byte aligned."""
    x = M.random_words((3, 70001), 0xF166, kind)
    x[2] = M.normal_words((70001,), 0xF167, kind)
    for k in (1, 65, 1000, 70001 // 4 + 1, 70001):
        for largest in BOTH:
            check(ls, torch_gpu, x, k, largest, kind, in_off=in_off, out_off=out_off)
    xs = M.random_words((5, 300), 0xF168, kind)  # short rows
    check(ls, torch_gpu, xs, 7, True, kind, in_off=in_off, out_off=out_off)


@KINDS
def test_output_directly_behind_the_input(ls, torch_gpu, kind):
    """One storage: the input's 2-byte elements, then the output's.  Extents of 4 bytes per key
    would make the two overlap."""
    torch = torch_gpu
    for rows, cols, k in ((3, 70001, 65), (5, 300, 7)):
        x = M.random_words((rows, cols), 0xF169, kind)
        n = rows * cols
        store = torch.zeros(n + rows * k, dtype=torch.int16, device="cuda")
        store[:n].copy_(torch.from_numpy(x.reshape(-1).view(np.int16)))
        d, ko = store[:n].view(rows, cols), store[n:].view(rows, k)
        io = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
        ls.topk_device(d, rows, cols, k, ko, io, largest=True, key=kind, workspace=ws)
        ls.topk_workspace_status(ws)
        ek, ei = M.topk_expected(x, k, True, kind)
        M.assert_keys(ko.cpu().numpy().view(np.uint16), ek, kind)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei)
        np.testing.assert_array_equal(d.cpu().numpy().view(np.uint16), x)


DCOLS = 200003  # odd (row 1 starts unaligned), 13 chunks


def dist_rows(name, kind):
    rng = np.random.default_rng(0xF16A)
    n, S = DCOLS, M.specials(kind)
    if name == "normal":
        return M.normal_words((2, n), 1, kind)
    if name == "all_nan":      # never narrows; positions must come out 0 .. k-1
        x = np.full((2, n), S["qnan"], dtype=np.uint16)
        x[:, 1::2] = S["-qnan1"]
        x[:, 2::7] = S["snan"]
        x[:, 3::11] = S["-snan"]
        return x
    if name == "neg_zero":
        return np.full((2, n), S["-0"], dtype=np.uint16)
    if name == "zeros":        # half -0.0, half +0.0
        return np.where(rng.random((2, n)) < 0.5, np.uint16(S["-0"]), np.uint16(S["+0"])).astype(np.uint16)
    if name in ("infs", "infs_rev"):  # 6 % of one infinity, 92 % of the other, the rest random
        lo, hi = (S["-inf"], S["+inf"]) if name == "infs" else (S["+inf"], S["-inf"])
        x = M.random_words((2, n), 5, kind)
        r = rng.random((2, n))
        x[r < 0.06] = lo
        x[r > 0.08] = hi
        return x
    if name == "mantissa":     # one sign and exponent, random mantissas: no bucket of level 0 fits the
        # candidate buffer, so level 1 counts over the raw 16-bit input
        mbits = 7 if kind == "bf16" else 10
        one = 0x3F80 if kind == "bf16" else 0x3C00
        return ((M.random_words((2, n), 7, kind, plant=False) & np.uint16((1 << mbits) - 1)) | np.uint16(one)).astype(np.uint16)
    raise ValueError(name)


@KINDS
@pytest.mark.parametrize("name", ["normal", "all_nan", "neg_zero", "zeros", "infs", "infs_rev", "mantissa"])
def test_distributions(ls, torch_gpu, name, kind):
    x = dist_rows(name, kind)
    S = M.specials(kind)
    ks = (1, 1000, 20000, DCOLS // ls.TOPK_SORT_DIV)
    assert max(ks) * ls.TOPK_SORT_DIV <= DCOLS  # the select runs
    for largest in BOTH:
        for k in ks:
            gk, gi = check(ls, torch_gpu, x, k, largest, kind)
            if name in ("all_nan", "neg_zero"):
                np.testing.assert_array_equal(gi, np.tile(np.arange(k, dtype=np.uint32), (2, 1)))
            if name == "zeros":  # every -0.0 first when ascending, last when descending
                want, other = (S["-0"], S["+0"]) if not largest else (S["+0"], S["-0"])
                nfirst = np.minimum((x == want).sum(axis=1), k)
                for r in range(2):
                    assert np.all(gk[r, :nfirst[r]] == want) and np.all(gk[r, nfirst[r]:] == other)


@KINDS
def test_nan_ties_at_the_threshold(ls, torch_gpu, kind):
    """30 % NaN: with largest the NaNs come first, so the k-th key is a NaN and the NaN ties taken are
    those with the lowest positions; a run of NaNs lies across a chunk boundary and k cuts inside it."""
    rng = np.random.default_rng(0xF16B)
    S = M.specials(kind)
    x = M.normal_words((2, DCOLS), 8, kind)
    r = rng.random((2, DCOLS))
    x[r < 0.15] = S["qnan"]
    x[(r >= 0.15) & (r < 0.30)] = S["-qnan1"]
    bounds = (CHUNK, 2 * CHUNK)
    for row, b in enumerate(bounds):
        x[row, b - 5:b + 6] = S["snan"]  # 11 NaN ties around the boundary
    nan = M.is_nan16(x, kind)
    # k = NaNs before the run + 6: the last one taken is the first word past the boundary (row 0)
    k_cut = int(nan[0, :CHUNK - 5].sum()) + 6
    assert k_cut * ls.TOPK_SORT_DIV <= DCOLS
    for k in (1, 1000, k_cut, 20000, DCOLS // ls.TOPK_SORT_DIV):
        gk, gi = check(ls, torch_gpu, x, k, True, kind)
        assert np.all(M.is_nan16(gk, kind))
        for row in range(2):
            np.testing.assert_array_equal(gi[row], np.flatnonzero(nan[row])[:k])
    _, gi = run(ls, torch_gpu, x, k_cut, True, kind)
    assert list(gi[0, -6:]) == list(range(CHUNK - 5, CHUNK + 1))
    # ascending, k past the non-NaN count: the tail of the output is the first NaNs (whole-row sort path)
    k = int((~nan[0]).sum()) + 10
    gk, gi = check(ls, torch_gpu, x[:1], k, False, kind)
    np.testing.assert_array_equal(gi[0, -10:], np.flatnonzero(nan[0])[:10])


@KINDS
@pytest.mark.parametrize("rows,cols,k", [(300, 257, 9), (3, 70001, 65), (1, 70001, 40000)])
def test_without_indices(ls, torch_gpu, rows, cols, k, kind):
    x = M.random_words((rows, cols), 0xF16C, kind)
    x[:, ::3] = M.tie_words((rows, cols), 3, kind)[:, ::3]
    gk, _ = run(ls, torch_gpu, x, k, True, kind)
    nk, none = run(ls, torch_gpu, x, k, True, kind, with_idx=False)
    assert none is None
    M.assert_keys(nk, gk, kind)
    M.assert_keys(nk, M.topk_expected(x, k, True, kind)[0], kind)


def run32(ls, torch, x, k, largest, key, ws):
    rows, cols = x.shape
    d = torch.from_numpy(x.view(np.int32)).cuda()
    ko = torch.full((rows, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    io = torch.full((rows, k), -7, dtype=torch.int32, device="cuda")
    ls.topk_device(d, rows, cols, k, ko, io, largest=largest, key=key, workspace=ws)
    ls.topk_workspace_status(ws)
    return ko.cpu().numpy().view(np.uint32), io.cpu().numpy().view(np.uint32)


def expected32(x, k, largest, key):
    if key == "f32":
        return F.topk_expected(x, k, largest)
    u = x ^ np.uint32((0x80000000 if key == "i32" else 0) ^ (0xFFFFFFFF if largest else 0))
    idx = np.argsort(u, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def test_workspace_reused_across_key_types(ls, torch_gpu):
    torch = torch_gpu
    calls = [((3, 70001), 1000, "bf16", False), ((2, 50000), 77, "i32", True), ((40, 300), 300, "f16", True),
             ((1, 70001), 60000, "u32", True), ((3, 70001), 1000, "f32", True), ((2, 40000), 9, "f16", False),
             ((1, 70001), 60000, "bf16", False), ((3, 70001), 1000, "f16", True), ((40, 300), 5, "bf16", False),
             ((2, 50000), 77, "bf16", True)]
    size = max(ls.topk_workspace_bytes(s[0], s[1], k) for s, k, *_ in calls)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (shape, k, key, largest) in enumerate(calls):
        if key in M.KINDS:
            x = M.tie_words(shape, 0xF16D + i, key) if i % 2 else M.random_words(shape, 0xF16D + i, key)
            check(ls, torch, x, k, largest, key, ws=ws)
            continue
        x = F.tie_words(shape, 0xF16D + i) if i % 2 else F.random_words(shape, 0xF16D + i)
        ek, ei = expected32(x, k, largest, key)
        gk, gi = run32(ls, torch, x, k, largest, key, ws)
        if key == "f32":
            F.assert_keys(gk, ek)
        else:
            np.testing.assert_array_equal(gk, ek)
        np.testing.assert_array_equal(gi, ei)


@KINDS
@pytest.mark.parametrize("rows,cols,k", [(2, 100003, 500), (4, 3000, 10)])
def test_graph_replay(ls, torch_gpu, rows, cols, k, kind):
    """One captured call replayed on new keys in the same buffers."""
    torch = torch_gpu
    dt = tdtype(torch, kind)
    src = torch.zeros((rows, cols), dtype=dt, device="cuda")
    ko = torch.zeros((rows, k), dtype=dt, device="cuda")
    io = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.topk_device(src, rows, cols, k, ko, io, largest=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.topk_device(src, rows, cols, k, ko, io, largest=True, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    S = M.specials(kind)
    inputs = {"normal": M.normal_words((rows, cols), 0xF16E, kind),
              "all_nan": np.full((rows, cols), S["-qnan1"], dtype=np.uint16),
              "const": np.full((rows, cols), 0xC049 if kind == "bf16" else 0xC248, dtype=np.uint16),
              "random_bits": M.random_words((rows, cols), 0xF16F, kind)}
    for dist, x in inputs.items():
        src.view(torch.int16).copy_(torch.from_numpy(x.view(np.int16)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.topk_workspace_status(ws)
        ek, ei = M.topk_expected(x, k, True, kind)
        M.assert_keys(ko.view(torch.int16).cpu().numpy().view(np.uint16), ek, kind, dist)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=dist)


@KINDS
@pytest.mark.parametrize("shape,k,gen", [((300, 257), 128, "ties"), ((3, 70001), 1000, "random"), ((2, DCOLS), 20000, "normal")])
def test_values_match_torch_topk(ls, torch_gpu, shape, k, gen, kind):
    """Values only (torch leaves the tie order open): equal, or both NaN, against torch.topk on the CPU
    tensor of the same dtype."""
    torch = torch_gpu
    x = {"ties": M.tie_words, "random": M.random_words, "normal": M.normal_words}[gen](shape, 0xF170, kind)
    t = M.to_torch(x, kind, torch)
    for largest in BOTH:
        gk, _ = run(ls, torch, x, k, largest, kind)
        want = torch.topk(t, k, dim=1, largest=largest, sorted=True).values.float().numpy()
        got = M.as_float32(gk, kind)
        assert np.all((got == want) | (np.isnan(got) & np.isnan(want))), (kind, shape, k, largest)


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("key", ["i32", "f32", "bf16", "f16"])
def test_topk_convenience(ls, torch_gpu, key, largest):
    """ls.topk on (3, 70001) and on one 1-D row: values of the input's dtype, int32 indices, against
    the models."""
    torch = torch_gpu
    rows, cols, k = 3, 70001, 65
    if key in M.KINDS:
        x = M.random_words((rows, cols), 0xF171, key)
        t = M.to_torch(x, key, torch).cuda()
        ek, ei = M.topk_expected(x, k, largest, key)
        words = lambda v: v.view(torch.int16).cpu().numpy().view(np.uint16)
        same = lambda g, e: M.assert_keys(g, e, key)
    else:
        x = F.random_words((rows, cols), 0xF171)
        t = torch.from_numpy(x.view(np.float32 if key == "f32" else np.int32)).cuda()
        ek, ei = expected32(x, k, largest, key)
        words = lambda v: v.view(torch.int32).cpu().numpy().view(np.uint32)
        same = F.assert_keys if key == "f32" else np.testing.assert_array_equal
    before = t.clone()
    values, indices = ls.topk(t, k, largest=largest)
    assert values.dtype == t.dtype and values.shape == (rows, k) and values.is_cuda
    assert indices.dtype == torch.int32 and indices.shape == (rows, k)
    same(words(values), ek)
    np.testing.assert_array_equal(indices.cpu().numpy().view(np.uint32), ei)
    v1, i1 = ls.topk(t[1], k, largest=largest)  # a 1-D tensor counts as one row
    assert v1.shape == (1, k) and i1.shape == (1, k)
    same(words(v1), ek[1:2])
    np.testing.assert_array_equal(i1.cpu().numpy().view(np.uint32), ei[1:2])
    assert torch.equal(t.view(torch.int16), before.view(torch.int16))
    if largest:  # the default direction is torch.topk's
        vd, idd = ls.topk(t, k)
        assert torch.equal(vd.view(torch.int16), values.view(torch.int16)) and torch.equal(idd, indices)
    with pytest.raises(TypeError):
        ls.topk(t.t(), k)
