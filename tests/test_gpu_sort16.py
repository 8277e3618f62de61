"""labsort_sort16_device on the GPU: whole output arrays (keys and positions) against the numpy model
of the contract (tests/rowsort_model.py over f16_model: the stable argsort of u(key)), for both
16-bit key types, at the smallest shapes at which the long path -- two radix passes over chunks of
C = sort16_chunk_keys() keys, a count table scanned along the chunks -- can go wrong.  Keys compare
bit-exact except that a NaN only has to be a NaN, positions exactly.  Every call runs on a workspace
filled with 0xFF and on outputs filled with a pattern with guard elements on each side, is followed
by the status call, and must leave its input as it was."""
import numpy as np
import pytest

import f16_model as M
import rowsort_model as R
import sort_sweep_model as S

pytestmark = pytest.mark.gpu

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", M.KINDS)
TDT = {"bf16": "bfloat16", "f16": "float16"}
KPAT, IPAT = 0x5A5A, -7


def tdtype(torch, kind):
    return getattr(torch, TDT[kind])


def run(ls, torch, x, descending, kind, ws=None, with_idx=True, in_off=0, out_off=0, entry="sort16"):
    """in_off / out_off: elements between the start of the storage and the matrix (odd: a matrix at an
    address that is 2-byte but not 4-byte aligned).  The outputs sit between guard elements that must
    keep their pattern.  entry: "sort16", or "rows" for ls.sort_rows_device on the same buffers."""
    rows, cols = x.shape
    n = rows * cols
    store = torch.full((n + in_off + 1,), 0x1111, dtype=torch.int16, device="cuda")
    d = store[in_off:in_off + n].view(rows, cols)
    d.copy_(torch.from_numpy(np.array(x).view(np.int16)))  # (a writable copy: a shared case is read-only)
    before = store.clone()
    g0 = 2 + out_off  # guard elements in front of the key output
    ostore = torch.full((g0 + n + 1,), KPAT, dtype=torch.int16, device="cuda")
    ko = ostore[g0:g0 + n].view(rows, cols)
    istore = torch.full((n + 2,), IPAT, dtype=torch.int32, device="cuda")
    io = istore[1:1 + n].view(rows, cols) if with_idx else None
    if ws is None:
        size = ls.sort16_workspace_bytes(rows, cols, with_idx) if entry == "sort16" else ls.sort_rows_workspace_bytes(rows, cols)
        ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 4 == 2 * (in_off % 2) and ko.data_ptr() % 4 == 2 * (out_off % 2)
    dt = tdtype(torch, kind)
    if entry == "sort16":
        ls.sort16_device(d.view(dt), rows, cols, ko.view(dt), io, descending=descending, key=kind, workspace=ws)
        ls.sort16_workspace_status(ws)
    else:
        ls.sort_rows_device(d.view(dt), rows, cols, ko.view(dt), io, descending=descending, key=kind, workspace=ws)
        ls.sort_rows_workspace_status(ws)
    assert torch.equal(store, before), "the input was written"
    assert bool((ostore[:g0] == KPAT).all()) and int(ostore[-1]) == KPAT, "written outside the key output"
    assert int(istore[0]) == IPAT and int(istore[-1]) == IPAT, "written outside the position output"
    if not with_idx:
        assert bool((istore == IPAT).all())
    gk = ko.cpu().numpy().view(np.uint16)
    return gk, (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, descending, kind, exp=None, with_idx=True, **kw):
    ek, ei = exp if exp is not None else R.expected(x, descending, kind)
    gk, gi = run(ls, torch, x, descending, kind, with_idx=with_idx, **kw)
    msg = f"{kind} {x.shape} descending={descending} idx={with_idx}"
    R.assert_keys(gk, ek, kind, msg)
    if with_idx:
        np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    return gk, gi


@KINDS
@pytest.mark.parametrize("cols", [32768, 32769])
def test_path_edge(ls, torch_gpu, cols, kind):
    """32768: the last row length forwarded to the LDS kernels (on a 256-byte workspace); 32769: the
    first long row, whose last chunk holds one key."""
    assert ls.segment_tile_keys() == 32768 and 32768 % ls.sort16_chunk_keys() == 0
    assert (ls.sort16_workspace_bytes(2, cols) == 256) == (cols == 32768)
    x, exp = R.case(kind, 2, cols)
    for desc in BOTH:
        check(ls, torch_gpu, x, desc, kind, exp=exp[desc])


@KINDS
@pytest.mark.parametrize("which", ["2C", "2C+1", "3C-1", "3C"])
def test_chunk_edges(ls, torch_gpu, which, kind):
    """Whole chunks only, one key behind them, one key short of them; 3 rows.  (2C at C = 16384 is
    the tile, the last forwarded length: 3C is the long path's first whole number of chunks.)"""
    C = ls.sort16_chunk_keys()
    cols = {"2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1, "3C": 3 * C}[which]
    x, exp = R.case(kind, 3, cols)
    for desc in BOTH:
        for with_idx in (True, False):
            check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=with_idx)


@KINDS
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_odd_rows(ls, torch_gpu, in_off, out_off, kind):
    """(2, 70001): consecutive rows start on both 2-byte phases of a 4-byte word; the matrix at the
    start of its storage and one element into it, for the input, the output and both."""
    x, exp = R.case(kind, 2, 70001)
    for desc in BOTH:
        check(ls, torch_gpu, x, desc, kind, exp=exp[desc], in_off=in_off, out_off=out_off)
    check(ls, torch_gpu, x, True, kind, exp=exp[True], with_idx=False, in_off=in_off, out_off=out_off)


@KINDS
def test_many_rows_few_chunks(ls, torch_gpu, kind):
    """(67, 32769): the scan's many-rows shape (a thread per (row, digit), one row per workgroup of
    the scan, so 67 workgroups), every row's last chunk one key long."""
    x, exp = R.case(kind, 67, 32769)
    check(ls, torch_gpu, x, True, kind, exp=exp[True])


def test_one_row_many_chunks(ls, torch_gpu):
    """One row of 1025 C + 5 keys (16.8 M at C = 16384), bfloat16, ascending, with positions: the scan
    of one (row, digit) by a workgroup takes a full 1024-wide step, then a partial step of two chunks
    (the last chunk five keys long)."""
    torch = torch_gpu
    C = ls.sort16_chunk_keys()
    cols = 1025 * C + 5
    x = M.random_words((1, cols), 0x5161, "bf16")
    x[0, 1000:cols:997] = M.specials("bf16")["-qnan1"]
    x[0, ::4099] = x[0, 7]
    check(ls, torch, x, False, "bf16")


@pytest.mark.parametrize("extra", [0, 1])
def test_scan_edge(ls, torch_gpu, extra):
    """One row of 64 C and of 64 C + 1 keys, bfloat16, descending, with positions: the most chunks that
    a thread per (row, digit) walks, and the fewest that a workgroup per (row, digit) scans, in one
    partial step, the last chunk one key long."""
    C = ls.sort16_chunk_keys()
    cols = 64 * C + extra
    x = M.random_words((1, cols), 0x5163 + extra, "bf16")
    x[0, 1000:cols:997] = M.specials("bf16")["-qnan1"]
    x[0, ::4099] = x[0, 7]
    check(ls, torch_gpu, x, True, "bf16")


@KINDS
@pytest.mark.parametrize("what", ["all_equal", "all_nan", "low_byte_equal", "high_byte_equal"])
def test_degenerate_digits(ls, torch_gpu, what, kind):
    """cols = 2C + 1, 2 rows.  One bin holds a whole chunk in both passes (all equal, all NaN) or in
    one of them; equal keys must keep position order in both directions."""
    torch = torch_gpu
    C = ls.sort16_chunk_keys()
    cols = 2 * C + 1
    assert cols > ls.segment_tile_keys()  # the long path
    rng = np.random.default_rng(0x5162)
    s = M.specials(kind)
    if what == "all_equal":
        x = np.empty((2, cols), dtype=np.uint16)
        x[0], x[1] = 0x3C5A, 0xBC01  # one positive and one negative finite value
    elif what == "all_nan":
        nans = np.array([s["qnan"], s["-qnan1"], s["snan"], s["-snan"], 0x7FFF, 0xFFFF], dtype=np.uint16)
        x = nans[rng.integers(0, nans.size, size=(2, cols))]
    elif what == "low_byte_equal":  # positive finite words: the image keeps the low byte
        x = ((rng.integers(0, 0x7C, size=(2, cols)) << 8) | 0x5A).astype(np.uint16)
    else:
        x = (0x3C00 | rng.integers(0, 256, size=(2, cols))).astype(np.uint16)
    assert not (what != "all_nan" and M.is_nan16(x, kind).any())
    for desc in BOTH:
        gk, gi = check(ls, torch, x, desc, kind)
        if what in ("all_equal", "all_nan"):
            np.testing.assert_array_equal(gi, np.broadcast_to(np.arange(cols, dtype=np.uint32), (2, cols)))
        if what == "all_nan":
            assert bool((gk == 0x7FFF).all())
        u = R.u_of(np.take_along_axis(x, gi.astype(np.int64), axis=1), kind, desc).astype(np.int64)
        assert bool((np.diff(u, axis=1) >= 0).all())
        tie = np.diff(u, axis=1) == 0
        assert bool((np.diff(gi.astype(np.int64), axis=1)[tie] > 0).all()), "equal keys out of position order"


@KINDS
@pytest.mark.parametrize("shape", ["2x70001", "3x(2C+1)"])
def test_agrees_with_the_row_sort(ls, torch_gpu, shape, kind):
    """Keys and positions bit-identical, NaN words included, to ls.sort_rows_device on the same input."""
    C = ls.sort16_chunk_keys()
    rows, cols = (2, 70001) if shape == "2x70001" else (3, 2 * C + 1)
    x, exp = R.case(kind, rows, cols)
    for desc in BOTH:
        k1, i1 = check(ls, torch_gpu, x, desc, kind, exp=exp[desc])
        k2, i2 = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], entry="rows")
        np.testing.assert_array_equal(k1, k2)
        np.testing.assert_array_equal(i1, i2)


@pytest.mark.parametrize("seed", S.SORT16_SEEDS)
def test_seeded_sweep(ls, torch_gpu, seed):
    """16 cases per seed (sort_sweep_model.sort16_sweep_cases): both key types, 1 to 4 long rows of up to
    6 C keys, half of the widths a whole number of chunks +-1, both directions, with and without
    positions, either 2-byte phase of input and output, through labsort_sort16_device or through
    labsort_sort_rows_device (whose outputs must then equal the first entry's bit for bit), every row
    from its own generator: among them rows whose images differ in one byte only, so that one radix
    pass puts whole chunks into one bin.  One workspace per seed, filled with 0xFF once and never
    cleared between the cases."""
    torch = torch_gpu
    C = ls.sort16_chunk_keys()
    cases = list(S.sort16_sweep_cases(seed, C, ls.segment_tile_keys()))
    size = max(max(ls.sort16_workspace_bytes(c["rows"], c["cols"], True), ls.sort_rows_workspace_bytes(c["rows"], c["cols"]))
               for c in cases)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    failures, hit = [], {}
    for i, c in enumerate(cases):
        for what in (c["entry"], c["kind"], f"edge {c['edge']}"):
            hit[what] = hit.get(what, 0) + 1
        kw = dict(ws=ws, with_idx=c["with_idx"], in_off=c["in_off"], out_off=c["out_off"])
        try:
            exp = R.expected(c["x"], c["descending"], c["kind"])
            k1, i1 = check(ls, torch, c["x"], c["descending"], c["kind"], exp=exp, entry="sort16", **kw)
            if c["entry"] == "rows":
                k2, i2 = check(ls, torch, c["x"], c["descending"], c["kind"], exp=exp, entry="rows", **kw)
                np.testing.assert_array_equal(k1, k2, err_msg="keys of the two entries")
                if c["with_idx"]:
                    np.testing.assert_array_equal(i1, i2, err_msg="positions of the two entries")
        except AssertionError as err:
            failures.append(f"seed {seed} case {i}: {c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {seed}: {dict(sorted(hit.items()))}")
    assert not failures, failures


@KINDS
def test_keys_only(ls, torch_gpu, kind):
    """d_idx_out = None writes the same keys as the call with positions."""
    x, exp = R.case(kind, 2, 70001)
    for desc in BOTH:
        k1, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=True)
        k0, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=False)
        np.testing.assert_array_equal(k1, k0)


def test_one_workspace_reused(ls, torch_gpu):
    """A sequence of calls that mix key types, directions, with and without positions and both paths
    on one workspace, never cleared between them."""
    torch = torch_gpu
    seq = [("bf16", 5, 300, True), ("f16", 2, 70001, True), ("bf16", 2, 32768, True), ("bf16", 2, 70001, False),
           ("f16", 3, 4097, False), ("f16", 2, 32769, True), ("bf16", 2, 70001, True), ("f16", 2, 32769, False),
           ("bf16", 9, 1025, True), ("f16", 2, 70001, False)]
    size = max(ls.sort16_workspace_bytes(r, c, True) for _, r, c, _ in seq)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (kind, rows, cols, with_idx) in enumerate(seq):
        x, exp = R.case(kind, rows, cols)
        desc = bool(i & 1) ^ (i >= 6)
        check(ls, torch, x, desc, kind, exp=exp[desc], with_idx=with_idx, ws=ws)


@KINDS
def test_graph_replay(ls, torch_gpu, kind):
    """(2, 2C + 1) captured once on a side stream, with positions, descending, and replayed on four
    inputs in the same buffers.  The launch sequence is linear."""
    torch = torch_gpu
    C = ls.sort16_chunk_keys()
    rows, cols = 2, 2 * C + 1
    assert cols > ls.segment_tile_keys()  # the long path
    dt = tdtype(torch, kind)
    src = torch.zeros((rows, cols), dtype=dt, device="cuda")
    ko = torch.zeros((rows, cols), dtype=dt, device="cuda")
    io = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sort16_workspace_bytes(rows, cols, True),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.sort16_device(src, rows, cols, ko, io, descending=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.sort16_device(src, rows, cols, ko, io, descending=True, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    inputs = {"random": R.random_words((rows, cols), 0x5165, kind),
              "all_nan": np.full((rows, cols), R.nan_word(kind), dtype=np.uint16),
              "ties": R.tie_words((rows, cols), 0x5166, kind),
              "planted": R.planted_words((rows, cols), 0x5167, kind)}
    for dist, x in inputs.items():
        x = np.ascontiguousarray(x, dtype=np.uint16)
        src.view(torch.int16).copy_(torch.from_numpy(x.view(np.int16)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.sort16_workspace_status(ws)
        ek, ei = R.expected(x, True, kind)
        R.assert_keys(ko.view(torch.int16).cpu().numpy().view(np.uint16), ek, kind, dist)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=dist)


@KINDS
def test_python_sort_and_argsort(ls, torch_gpu, kind):
    """ls.sort / ls.argsort on a (2, 70001) tensor and on a 1-D tensor of 70001 elements: shapes,
    dtypes, values, positions, the input unwritten."""
    torch = torch_gpu
    x, exp = R.case(kind, 2, 70001)
    tg = M.to_torch(x, kind, torch).cuda()

    def words(t):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)

    v, i = ls.sort(tg)
    assert v.dtype == tg.dtype and i.dtype == torch.int32 and v.shape == tg.shape and i.shape == tg.shape
    R.assert_keys(words(v), exp[False][0], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[False][1])
    v, i = ls.sort(tg, descending=True)
    R.assert_keys(words(v), exp[True][0], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[True][1])
    np.testing.assert_array_equal(ls.argsort(tg).cpu().numpy().view(np.uint32), exp[False][1])
    np.testing.assert_array_equal(ls.argsort(tg, descending=True).cpu().numpy().view(np.uint32), exp[True][1])
    row = tg[1].contiguous()  # 1-D: one row, the whole-array sort
    v, i = ls.sort(row)
    assert v.shape == (70001,) and i.shape == (70001,) and v.dtype == tg.dtype and i.dtype == torch.int32
    R.assert_keys(words(v), exp[False][0][1], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[False][1][1])
    v, i = ls.sort(row, descending=True)
    R.assert_keys(words(v), exp[True][0][1], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[True][1][1])
    a = ls.argsort(row, descending=True)
    assert a.shape == (70001,)
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), exp[True][1][1])
    assert torch.equal(tg.view(torch.int16).cpu(), M.to_torch(x, kind, torch).view(torch.int16)), "the input was written"


@KINDS
def test_python_route_by_timing_class(ls, torch_gpu, kind):
    """With the timing hooks on, ls.sort of long 16-bit rows launches under LABSORT_K_SEGSORT and not
    under LABSORT_K_TOPK, which is what tells the new route from the row sort's; with a caller's
    workspace (sized for the row sort) the old route stays."""
    torch = torch_gpu
    x, exp = R.case(kind, 2, 70001)
    tg = M.to_torch(x, kind, torch).cuda()
    ls.timing_enable(True)
    try:
        v, i = ls.sort(tg, descending=True)
        torch.cuda.synchronize()
        seg, topk = ls.timing_read("segsort"), ls.timing_read("topk")
        assert seg[1] >= 1 and topk[1] == 0, (seg, topk)
        ls.timing_enable(True)  # clears
        ws = torch.full((ls.sort_rows_workspace_bytes(2, 70001),), 0xFF, dtype=torch.uint8, device="cuda")
        v2, i2 = ls.sort(tg, descending=True, workspace=ws)
        ls.sort_rows_workspace_status(ws)
        assert ls.timing_read("topk")[1] >= 1
    finally:
        ls.timing_enable(False)
    assert torch.equal(v.view(torch.int16), v2.view(torch.int16)) and torch.equal(i, i2)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[True][1])
