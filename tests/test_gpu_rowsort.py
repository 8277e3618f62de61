"""labsort_sort_rows_device on the GPU: whole output arrays (keys and positions) against the numpy
models of the contract (tests/rowsort_model.py over f16_model / f32_model: the stable argsort of
u(key)), for the five key types, both directions, with and without positions, across the edges of
the LDS classes and of the two tiles, on the long path behind them, on rows whose keys differ in
every chosen set of digits (tests/sort_sweep_model.py) and in a seeded sweep.  Keys compare bit-exact
except that a NaN only has to be a NaN, positions exactly.  Every call runs on a workspace filled
with 0xFF and on outputs filled with a pattern with a guard element on each side, is followed by
the status call, and must leave its input as it was."""
import numpy as np
import pytest

import f16_model as M
import rowsort_model as R
import sort_sweep_model as S

pytestmark = pytest.mark.gpu

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", R.KINDS)
KINDS16 = pytest.mark.parametrize("kind", M.KINDS)
TDT = {"u32": "int32", "i32": "int32", "f32": "float32", "bf16": "bfloat16", "f16": "float16"}
KPAT, IPAT = 0x5A5A, -7


def tdtype(torch, kind):
    return getattr(torch, TDT[kind])


def run(ls, torch, x, descending, kind, ws=None, with_idx=True, in_off=0, out_off=0):
    """in_off / out_off: elements between the start of the storage and the matrix (odd: a 16-bit
    matrix at an address that is 2-byte but not 4-byte aligned).  The outputs sit between guard
    elements that must keep their pattern."""
    rows, cols = x.shape
    n = rows * cols
    sdt = torch.int16 if R.is16(kind) else torch.int32
    npdt = np.int16 if R.is16(kind) else np.int32
    store = torch.full((n + in_off + 1,), 0x1111, dtype=sdt, device="cuda")
    d = store[in_off:in_off + n].view(rows, cols)
    d.copy_(torch.from_numpy(np.array(x).view(npdt)))  # (a writable copy: a shared case is read-only)
    before = store.clone()
    g0 = 2 + out_off  # guard elements in front of the key output
    ostore = torch.full((g0 + n + 1,), KPAT, dtype=sdt, device="cuda")
    ko = ostore[g0:g0 + n].view(rows, cols)
    istore = torch.full((n + 2,), IPAT, dtype=torch.int32, device="cuda")
    io = istore[1:1 + n].view(rows, cols) if with_idx else None
    if ws is None:
        ws = torch.full((ls.sort_rows_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    if R.is16(kind):
        assert d.data_ptr() % 4 == 2 * (in_off % 2) and ko.data_ptr() % 4 == 2 * (out_off % 2)
    dt = tdtype(torch, kind)
    ls.sort_rows_device(d.view(dt), rows, cols, ko.view(dt), io, descending=descending, key=kind, workspace=ws)
    ls.sort_rows_workspace_status(ws)
    assert torch.equal(store, before), "the input was written"
    assert bool((ostore[:g0] == KPAT).all()) and int(ostore[-1]) == KPAT, "written outside the key output"
    assert int(istore[0]) == IPAT and int(istore[-1]) == IPAT, "written outside the position output"
    if not with_idx:
        assert bool((istore == IPAT).all())
    gk = ko.cpu().numpy().view(R.wdtype(kind))
    return gk, (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, descending, kind, exp=None, with_idx=True, **kw):
    ek, ei = exp if exp is not None else R.expected(x, descending, kind)
    gk, gi = run(ls, torch, x, descending, kind, with_idx=with_idx, **kw)
    msg = f"{kind} {x.shape} descending={descending} idx={with_idx}"
    R.assert_keys(gk, ek, kind, msg)
    if with_idx:
        np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    return gk, gi


def check_all(ls, torch, kind, rows, cols, gen="mixed", **kw):
    """Both directions, with and without positions, on one shared case."""
    x, exp = R.case(kind, rows, cols, gen)
    for desc in BOTH:
        for with_idx in (True, False):
            check(ls, torch, x, desc, kind, exp=exp[desc], with_idx=with_idx, **kw)


def lds_path(ls, cols, kind, with_idx):
    return cols <= (ls.segment_tile_keys() if (R.is16(kind) or not with_idx) else ls.segment_pair_tile_keys())


def test_class_edges_are_the_segmented_sorts(ls):
    assert ls.segment_class_edges(False) == [256, 512, 1024, 4096, 32768]
    assert ls.segment_class_edges(True) == [256, 512, 1024, 4096, 16384]


@KINDS
@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 4096, 4097])
def test_class_edges(ls, torch_gpu, cols, kind):
    """Both sides of every class edge below the tile; 3 to 300 rows (never a multiple of the four
    rows a wave-class workgroup takes)."""
    rows = max(3, min(299, 150000 // cols))
    check_all(ls, torch_gpu, kind, rows, cols)


@KINDS
@pytest.mark.parametrize("cols", [16384, 16385, 32767, 32768, 32769])
def test_tile_edges(ls, torch_gpu, cols, kind):
    """Across the pair tile (32-bit keys with positions change path at 16385) and the tile
    (everything changes path at 32769)."""
    rows = 3 if cols <= 16385 else 2
    assert lds_path(ls, cols, kind, True) == (cols <= (32768 if R.is16(kind) else 16384))
    assert lds_path(ls, cols, kind, False) == (cols <= 32768)
    check_all(ls, torch_gpu, kind, rows, cols)


GRID_SHAPES = [(9000, 65, 32), (9000, 257, 32), (4200, 513, 16), (1700, 1025, 6), (300, 4097, 1)]


@KINDS
@pytest.mark.parametrize("rows,cols,per_cu", GRID_SHAPES)
def test_grid_stride(ls, torch_gpu, rows, cols, per_cu, kind):
    """More rows than the class's fixed grid has waves / workgroups (csrc/rowsort.hip's launch_rs: 8, 8
    and 4 workgroups of four waves per CU for the wave classes, 6 workgroups per CU for the block
    class, one for the tile class), so a kernel that loops over rows runs its loop more than once.
    (The classes that take one wave / workgroup per row by default loop in test_grid_forms.)"""
    torch = torch_gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rows > per_cu * cus, (rows, per_cu, cus)
    x, exp = R.make_case(kind, rows, cols, "random")  # (used once: not kept)
    check(ls, torch, x, False, kind, exp=exp[False])
    check(ls, torch, x, True, kind, exp=exp[True], with_idx=(rows % 2 == 0))


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16"])
@pytest.mark.parametrize("form", ["rows", "fixed"])
@pytest.mark.parametrize("rows,cols,per_cu", GRID_SHAPES)
def test_grid_forms(ls, torch_gpu, monkeypatch, rows, cols, per_cu, form, kind):
    """Both grid forms of every class, forced (LABSORT_ROWSORT_GRID, read at every call): the fixed
    grid loops over the rows, the other has a wave / workgroup per row."""
    torch = torch_gpu
    assert rows > per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("LABSORT_ROWSORT_GRID", form)
    x, exp = R.make_case(kind, rows, cols, "random")
    check(ls, torch, x, True, kind, exp=exp[True])
    check(ls, torch, x, False, kind, exp=exp[False], with_idx=False)


@KINDS
@pytest.mark.parametrize("rows,cols", [(7, 200), (5, 3000), (2, 16384)])
def test_ties_nans_and_zeros(ls, torch_gpu, rows, cols, kind):
    """Rows of heavy ties (NaNs of both signs, quiet and signalling, -0.0 and +0.0 for the float
    types), and random rows with every special value planted."""
    torch = torch_gpu
    check_all(ls, torch, kind, rows, cols, "ties")
    x = R.planted_words((rows, cols), 0x5042 + cols, kind)
    for desc in BOTH:
        check(ls, torch, x, desc, kind)


@KINDS
@pytest.mark.parametrize("cols", [40, 300, 5000, 16384, 20000])
def test_all_equal_rows(ls, torch_gpu, cols, kind):
    """No digit differs in a row of one repeated value or of NaNs only: no pass runs (a packed
    word's position half must not start one) and the positions come out 0 .. cols - 1."""
    torch = torch_gpu
    x = np.empty((4, cols), dtype=R.wdtype(kind))
    x[0] = R.random_words((1,), 0x5043, kind)[0] & (0x3FFF if R.is16(kind) else 0x3FFFFFFF)  # one finite value
    x[1] = R.nan_word(kind)
    x[2] = 0
    x[3] = x[0]
    for desc in BOTH:
        for with_idx in (True, False):
            gk, gi = check(ls, torch, x, desc, kind, with_idx=with_idx)
            if with_idx:
                np.testing.assert_array_equal(gi, np.broadcast_to(np.arange(cols, dtype=np.uint32), (4, cols)))


@KINDS
@pytest.mark.parametrize("cols", [200, 1000, 4000, 16384, 32768])
def test_nans_beside_padding(ls, torch_gpu, cols, kind):
    """The last 40 keys of a row are NaNs (for the integer types: the largest key), whose image is
    the padding's: ascending they are the last 40 outputs, in position order, in a full tile
    (16384 pairs, 32768 keys) and beside the padding of a partly filled last group."""
    torch = torch_gpu
    x = R.random_words((2, cols), 0x5044 + cols, kind).astype(R.wdtype(kind))
    x[:, -40:] = R.nan_word(kind)
    x[1, :40] = R.nan_word(kind)
    for with_idx in (True, False):
        gk, gi = check(ls, torch, x, False, kind, with_idx=with_idx)
        if with_idx:
            np.testing.assert_array_equal(gi[0, -40:], np.arange(cols - 40, cols, dtype=np.uint32))
    check(ls, torch, x, True, kind)


@KINDS16
@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("rows,cols", [(9, 257), (5, 4097), (3, 63)])
def test_misaligned_16bit(ls, torch_gpu, rows, cols, in_off, out_off, kind):
    """Odd cols: consecutive rows start on both 2-byte phases of a 4-byte word; the matrix one
    element into its storage, for the input, the output and both."""
    x, exp = R.case(kind, rows, cols)
    for desc in BOTH:
        check(ls, torch_gpu, x, desc, kind, exp=exp[desc], in_off=in_off, out_off=out_off)
    check(ls, torch_gpu, x, True, kind, exp=exp[True], with_idx=False, in_off=in_off, out_off=out_off)


@KINDS16
@pytest.mark.parametrize("rows,cols", [(5, 257), (3, 4097), (2, 70001)])
def test_output_directly_behind_the_input(ls, torch_gpu, rows, cols, kind):
    """One storage: the input's 2-byte elements, then the output's.  Extents of 4 bytes per key
    would make the two overlap."""
    torch = torch_gpu
    x, exp = R.case(kind, rows, cols)
    n = rows * cols
    store = torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    store[:n].copy_(torch.from_numpy(np.array(x).reshape(-1).view(np.int16)))
    d, ko = store[:n].view(rows, cols), store[n:].view(rows, cols)
    io = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sort_rows_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sort_rows_device(d, rows, cols, ko, io, descending=True, key=kind, workspace=ws)
    ls.sort_rows_workspace_status(ws)
    R.assert_keys(ko.cpu().numpy().view(np.uint16), exp[True][0], kind)
    np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), exp[True][1])
    np.testing.assert_array_equal(d.cpu().numpy().view(np.uint16), x)


@KINDS
def test_long_path(ls, torch_gpu, kind):
    """(2, 70001): past both tiles, top-k's whole-row sort on the caller's workspace."""
    assert not lds_path(ls, 70001, kind, False)
    x, exp = R.case(kind, 2, 70001)
    for desc in BOTH:
        check(ls, torch_gpu, x, desc, kind, exp=exp[desc])
    check(ls, torch_gpu, x, True, kind, exp=exp[True], with_idx=False)


def test_paths_agree_between_the_tiles(ls, torch_gpu):
    """(2, 20000) int32: with positions the long path, without them the LDS path; the same keys."""
    kind = "i32"
    assert not lds_path(ls, 20000, kind, True) and lds_path(ls, 20000, kind, False)
    x, exp = R.case(kind, 2, 20000)
    for desc in BOTH:
        k1, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=True)
        k2, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=False)
        np.testing.assert_array_equal(k1, k2)


def test_one_workspace_reused(ls, torch_gpu):
    """A sequence of calls that mix key types, directions and paths on one workspace, never cleared
    between them."""
    torch = torch_gpu
    seq = [("bf16", 5, 300, True), ("i32", 2, 70001, True), ("f32", 3, 4097, True), ("f16", 2, 32768, True),
           ("u32", 2, 20000, True), ("u32", 2, 20000, False), ("bf16", 2, 70001, True), ("f32", 7, 65, False),
           ("i32", 3, 16385, True), ("f16", 9, 1025, True)]
    size = max(ls.sort_rows_workspace_bytes(r, c) for _, r, c, _ in seq)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (kind, rows, cols, with_idx) in enumerate(seq):
        x, exp = R.case(kind, rows, cols)
        desc = bool(i & 1)
        check(ls, torch, x, desc, kind, exp=exp[desc], with_idx=with_idx, ws=ws)


@pytest.mark.parametrize("kind", ["f32", "bf16", "i32", "f16"])
def test_graph_replay(ls, torch_gpu, kind):
    """One captured LDS-path call per key width replayed on new keys in the same buffers."""
    torch = torch_gpu
    rows, cols = 4, 3000
    dt = tdtype(torch, kind)
    sdt = torch.int16 if R.is16(kind) else torch.int32
    src = torch.zeros((rows, cols), dtype=dt, device="cuda")
    ko = torch.zeros((rows, cols), dtype=dt, device="cuda")
    io = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sort_rows_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.sort_rows_device(src, rows, cols, ko, io, descending=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.sort_rows_device(src, rows, cols, ko, io, descending=True, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    inputs = {"random": R.random_words((rows, cols), 0x5045, kind),
              "all_nan": np.full((rows, cols), R.nan_word(kind), dtype=R.wdtype(kind)),
              "ties": R.tie_words((rows, cols), 0x5046, kind),
              "planted": R.planted_words((rows, cols), 0x5047, kind)}
    for dist, x in inputs.items():
        x = np.ascontiguousarray(x, dtype=R.wdtype(kind))
        src.view(sdt).copy_(torch.from_numpy(x.view(np.int16 if R.is16(kind) else np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.sort_rows_workspace_status(ws)
        ek, ei = R.expected(x, True, kind)
        R.assert_keys(ko.view(sdt).cpu().numpy().view(R.wdtype(kind)), ek, kind, dist)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=dist)


@KINDS
@pytest.mark.parametrize("cols", [33, 64, 65, 200, 400, 900, 3000, 9000, 16384, 32768])
def test_digit_masks(ls, torch_gpu, cols, kind):
    """The pass-skip logic of every class: one matrix whose rows run through every set of differing
    digits (16 masks of four digits, 4 of a packed word's two) times every variant of
    sort_sweep_model.digit_mask_rows: digits random per key, digits of two values one bit apart, and
    all keys equal but the first, the last (beside the padding) or one in the middle (in another
    wave's stripe).  A kernel that skips a pass it needs, or lets a packed word's position half
    decide, orders a row wrongly; with only some passes run, equal keys must still come out in
    position order.  32768: the calls that stay in LDS at that length."""
    torch = torch_gpu
    x, labels = S.mask_matrix(kind, cols, 0x5048 + cols)
    assert x.shape[0] == (20 if R.is16(kind) else 80)
    np.testing.assert_array_equal(S.mask_of(R.u_of(x, kind)), [m for m, _ in labels])
    idx_forms = [w for w in (True, False) if lds_path(ls, cols, kind, w)]
    assert idx_forms == ([True, False] if R.is16(kind) or cols <= 16384 else [False])
    offs = [(0, 0), (1, 1)] if R.is16(kind) else [(0, 0)]
    for desc in BOTH:
        exp = R.expected(x, desc, kind)
        for with_idx in idx_forms:
            for in_off, out_off in offs:
                gk, gi = run(ls, torch, x, desc, kind, with_idx=with_idx, in_off=in_off, out_off=out_off)
                msg = f"{kind} cols={cols} descending={desc} idx={with_idx} offsets=({in_off}, {out_off})"
                # (no NaN among these keys: words compare as they are; the first wrong row by its name)
                bad = (gk != exp[0]).any(axis=1) | ((gi != exp[1]).any(axis=1) if with_idx else False)
                if bad.any():
                    r = int(np.flatnonzero(bad)[0])
                    raise AssertionError(f"{msg}: {int(bad.sum())} rows differ, the first is row {r}: "
                                         f"mask {labels[r][0]:#x} {labels[r][1]}")
                R.assert_keys(gk, exp[0], kind, msg)
                if with_idx:
                    np.testing.assert_array_equal(gi, exp[1], err_msg=f"positions {msg}")
                    S.assert_ties_in_position_order(x, gi, kind, desc, msg)


@pytest.mark.parametrize("seed", S.ROWSORT_SEEDS)
def test_seeded_sweep(ls, torch_gpu, monkeypatch, seed):
    """40 cases per seed (sort_sweep_model.rowsort_sweep_cases): the five key types, 1 to 48 rows, cols on
    the class and tile edges, log-uniform below the tile and past it, both directions, with and
    without positions, the grid form unset or forced, 16-bit matrices at either 2-byte phase, every
    row from its own generator (digit masks, ties, NaNs, sorted, all equal ...).  One workspace per
    seed, filled with 0xFF once and never cleared between the cases."""
    torch = torch_gpu
    e = ls.segment_class_edges(False)
    cases = list(S.rowsort_sweep_cases(seed, e[:-1], ls.segment_tile_keys(), ls.segment_pair_tile_keys()))
    size = max(ls.sort_rows_workspace_bytes(c["rows"], c["cols"]) for c in cases)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths = [], {}
    for i, c in enumerate(cases):
        assert (c["path"] != "long") == lds_path(ls, c["cols"], c["kind"], c["with_idx"]), c["tag"]
        paths[c["path"]] = paths.get(c["path"], 0) + 1
        if c["grid"] is None:
            monkeypatch.delenv("LABSORT_ROWSORT_GRID", raising=False)
        else:
            monkeypatch.setenv("LABSORT_ROWSORT_GRID", c["grid"])
        try:
            check(ls, torch, c["x"], c["descending"], c["kind"], ws=ws, with_idx=c["with_idx"], in_off=c["in_off"],
                  out_off=c["out_off"])
        except AssertionError as err:
            failures.append(f"seed {seed} case {i}: {c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {seed}: classes and paths {dict(sorted(paths.items()))}")
    assert not failures, failures


def to_torch(x, kind, torch):
    if R.is16(kind):
        return M.to_torch(x, kind, torch)
    t = torch.from_numpy(np.ascontiguousarray(x).view(np.int32).copy())
    return t.view(torch.float32) if kind == "f32" else t


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(37, 300), (5, 4097), (2, 70001)])
def test_cross_checks(ls, torch_gpu, rows, cols, kind):
    """Keys and positions equal ls.topk(x, cols); values equal torch.sort on the CPU tensor, compared
    as floats with NaN == NaN (torch's -0.0 == +0.0 leaves its indices incomparable)."""
    torch = torch_gpu
    x, exp = R.case(kind, rows, cols)
    t = to_torch(x, kind, torch)
    tg = t.cuda()
    for desc in BOTH:
        gk, gi = check(ls, torch, x, desc, kind, exp=exp[desc])
        tv, ti = ls.topk(tg, cols, largest=desc)
        torch.cuda.synchronize()
        sdt = torch.int16 if R.is16(kind) else torch.int32
        R.assert_keys(gk, tv.view(sdt).cpu().numpy().view(R.wdtype(kind)), kind, "against topk")
        np.testing.assert_array_equal(gi, ti.cpu().numpy().view(np.uint32))
        want = torch.sort(t, dim=1, descending=desc, stable=True).values
        if kind == "i32":
            np.testing.assert_array_equal(gk.view(np.int32), want.numpy())
        else:
            got = M.as_float32(gk, kind) if R.is16(kind) else gk.view(np.float32)
            want = want.float().numpy()
            assert np.all((got == want) | (np.isnan(got) & np.isnan(want))), (kind, rows, cols, desc)


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16", "f16"])
def test_python_convenience(ls, torch_gpu, kind):
    """ls.sort / ls.argsort: dtypes and shapes, the 1-D case, ascending by default."""
    torch = torch_gpu
    x, exp = R.case(kind, 6, 700)
    sdt = torch.int16 if R.is16(kind) else torch.int32
    tg = to_torch(x, kind, torch).cuda()
    v, i = ls.sort(tg)
    assert v.dtype == tg.dtype and i.dtype == torch.int32 and v.shape == tg.shape and i.shape == tg.shape
    R.assert_keys(v.view(sdt).cpu().numpy().view(R.wdtype(kind)), exp[False][0], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[False][1])
    v, i = ls.sort(tg, descending=True)
    R.assert_keys(v.view(sdt).cpu().numpy().view(R.wdtype(kind)), exp[True][0], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[True][1])
    np.testing.assert_array_equal(ls.argsort(tg).cpu().numpy().view(np.uint32), exp[False][1])
    np.testing.assert_array_equal(ls.argsort(tg, descending=True).cpu().numpy().view(np.uint32), exp[True][1])
    row = tg[2].contiguous()  # 1-D: one row
    v, i = ls.sort(row)
    assert v.shape == (700,) and i.shape == (700,) and v.dtype == tg.dtype and i.dtype == torch.int32
    R.assert_keys(v.view(sdt).cpu().numpy().view(R.wdtype(kind)), exp[False][0][2], kind)
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), exp[False][1][2])
    assert ls.argsort(row, descending=True).shape == (700,)
    assert torch.equal(tg.view(sdt).cpu(), to_torch(x, kind, torch).view(sdt)), "the input was written"
