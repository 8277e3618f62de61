"""labsort_sort64_device on the GPU: whole output arrays (keys and positions) bit for bit against the
numpy model of the contract (tests/sort64_model.py: the stable argsort of the image, keys taken
through the inverse image), for the three 8-byte key types and both directions, at the smallest
shapes at which either path -- one workgroup per row up to C = sort64_chunk_keys() keys, chunked
count / scan / scatter passes above -- can go wrong, and the plan the device made (sort64_passes)
against the set of bytes in which the images vary.  Every call runs on a workspace filled with 0xFF
and on outputs filled with a pattern with guard elements on each side, is followed by the status
call, and must leave its input as it was."""
import numpy as np
import pytest

import sort64_model as M

try:  # the dtypes ls.sort takes beyond the narrower ones: uint64 where the installed torch has it
    import torch as _torch
    DTYPES = ["int64", "float64"] + (["uint64"] if hasattr(_torch, "uint64") else [])
except ImportError:
    DTYPES = ["int64", "float64"]

pytestmark = pytest.mark.gpu

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", M.KINDS)
KPAT, IPAT = 0x5A5A5A5A5A5A5A5A, -7
# the sets every variant of the digit-mask test runs, as bitmasks: {}, {0}, {7}, {0, 7}, {3, 4}, all
# eight bytes, and six more
DOZEN = [0x00, 0x01, 0x80, 0x81, 0x18, 0xFF, 0x02, 0x24, 0x40, 0x0F, 0xF0, 0xAA]


def run(ls, torch, x, descending, kind, ws=None, with_idx=True, in_off=0, out_off=0):
    """in_off / out_off: elements between the start of the (256-byte aligned) storage and the matrix.
    The outputs sit between guard elements that must keep their pattern.  Returns the keys, the
    positions (or None) and sort64_passes."""
    rows, cols = x.shape
    n = rows * cols
    store = torch.full((n + in_off + 1,), 0x1111, dtype=torch.int64, device="cuda")
    d = store[in_off:in_off + n].view(rows, cols)
    d.copy_(torch.from_numpy(np.array(x).view(np.int64)))  # (a writable copy: a shared case is read-only)
    before = store.clone()
    g0 = 32 + out_off  # guard elements in front of the key output
    ostore = torch.full((g0 + n + 1,), KPAT, dtype=torch.int64, device="cuda")
    ko = ostore[g0:g0 + n].view(rows, cols)
    istore = torch.full((n + 2,), IPAT, dtype=torch.int32, device="cuda")
    io = istore[1:1 + n].view(rows, cols) if with_idx else None
    if ws is None:
        ws = torch.full((ls.sort64_workspace_bytes(rows, cols, with_idx),), 0xFF, dtype=torch.uint8, device="cuda")
    assert store.data_ptr() % 256 == 0 and ostore.data_ptr() % 256 == 0
    assert d.data_ptr() % 256 == 8 * in_off and ko.data_ptr() % 256 == 8 * out_off
    ls.sort64_device(d, rows, cols, ko, io, descending=descending, key=kind, workspace=ws)
    ls.sort64_workspace_status(ws)
    passes = ls.sort64_passes(ws)
    assert torch.equal(store, before), "the input was written"
    assert bool((ostore[:g0] == KPAT).all()) and int(ostore[-1]) == KPAT, "written outside the key output"
    assert int(istore[0]) == IPAT and int(istore[-1]) == IPAT, "written outside the position output"
    if not with_idx:
        assert bool((istore == IPAT).all())
    gk = ko.cpu().numpy().view(np.uint64)
    return gk, (io.cpu().numpy().view(np.uint32) if with_idx else None), passes


def check(ls, torch, x, descending, kind, exp=None, with_idx=True, **kw):
    ek, ei = exp if exp is not None else M.expected(x, descending, kind)
    gk, gi, passes = run(ls, torch, x, descending, kind, with_idx=with_idx, **kw)
    msg = f"{kind} {x.shape} descending={descending} idx={with_idx}"
    np.testing.assert_array_equal(gk, ek, err_msg=f"keys {msg}")
    if with_idx:
        np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    want = M.active_bytes(x, kind, descending) if x.shape[1] > ls.sort64_chunk_keys() else 0
    assert passes == want, f"passes {passes:#x}, the images vary in {want:#x}: {msg}"
    return gk, gi


def cols_of(ls, which):
    C = ls.sort64_chunk_keys()
    return {"1": 1, "2": 2, "63": 63, "64": 64, "65": 65, "1000": 1000, "C/4": C // 4, "C/4+1": C // 4 + 1, "C/2": C // 2,
            "C/2+1": C // 2 + 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1}[which]


@KINDS
@pytest.mark.parametrize("which", ["1", "2", "63", "64", "65", "1000", "C/4", "C/4+1", "C/2", "C/2+1", "C-1", "C", "C+1", "2C",
                                   "2C+1", "3C-1"])
def test_row_lengths(ls, torch_gpu, which, kind):
    """1 and 3 rows, both directions; without positions the same keys.  C/4 and C/2 are the longest rows
    that a workgroup of a quarter and of half the full size sorts."""
    cols = cols_of(ls, which)
    assert (ls.sort64_workspace_bytes(3, cols) == 256) == (cols <= ls.sort64_chunk_keys())
    for rows in (1, 3):
        x, exp = M.case(kind, rows, cols)
        for desc in BOTH:
            k1, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc])
            k0, _ = check(ls, torch_gpu, x, desc, kind, exp=exp[desc], with_idx=False)
            np.testing.assert_array_equal(k1, k0)


@KINDS
def test_many_rows(ls, torch_gpu, kind):
    """(67, C + 1): two chunks per row, the second one key long; the scan by a thread per (row, digit),
    67 workgroups of it."""
    C = ls.sort64_chunk_keys()
    x, exp = M.case(kind, 67, C + 1)
    check(ls, torch_gpu, x, True, kind, exp=exp[True])
    check(ls, torch_gpu, x, False, kind, exp=exp[False], with_idx=False)


def test_one_row_many_chunks(ls, torch_gpu):
    """One row of 65 chunks, the last one five keys long: the fewest chunks that the scan by a workgroup
    per (row, digit) takes (up to 64 a thread walks them)."""
    C = ls.sort64_chunk_keys()
    x = M.planted((1, 64 * C + 5), 0x6451, "f64")
    check(ls, torch_gpu, x, False, "f64")
    check(ls, torch_gpu, x, True, "i64", with_idx=False)


def test_one_row_64_chunks(ls, torch_gpu):
    """One row of exactly 64 chunks, u64, with positions: the most chunks that a thread per (row, digit)
    walks."""
    C = ls.sort64_chunk_keys()
    x = M.planted((1, 64 * C), 0x6452, "u64")
    check(ls, torch_gpu, x, False, "u64")


def test_rows_of_65_chunks(ls, torch_gpu):
    """(3, 64 C + 1), keys only: the scan by a workgroup per (row, digit) over more than one row, whose
    carry must stay inside its (row, digit); every row's last chunk one key long."""
    C = ls.sort64_chunk_keys()
    x = M.planted((3, 64 * C + 1), 0x6453, "u64")
    check(ls, torch_gpu, x, False, "u64", with_idx=False)


@pytest.mark.parametrize("part", range(4))
def test_digit_masks_long(ls, torch_gpu, part):
    """One row of 2C + 1 u64 keys whose images vary in exactly a chosen set of bytes, all 256 sets (64
    per case), ascending: the result, and sort64_passes equal to the set.  m = 0 .. 8 active passes:
    both parities of the ping-pong between the outputs and the temporaries, and k_s64_same."""
    C = ls.sort64_chunk_keys()
    ws = torch_gpu.full((ls.sort64_workspace_bytes(1, 2 * C + 1, True),), 0xFF, dtype=torch_gpu.uint8, device="cuda")
    for mask in range(64 * part, 64 * part + 64):
        x = M.rows_with_bytes((1, 2 * C + 1), mask, 0x6460 + mask, "u64")
        assert M.active_bytes(x, "u64") == mask
        check(ls, torch_gpu, x, False, "u64", ws=ws)  # (checks the passes against the set)


@pytest.mark.parametrize("part", range(4))
def test_digit_masks_lds(ls, torch_gpu, part):
    """The same 256 sets at 3 rows of 1000 keys, sorted by a workgroup per row in LDS: the plan is the
    row's own and sort64_passes reports 0."""
    for mask in range(64 * part, 64 * part + 64):
        x = M.rows_with_bytes((3, 1000), mask, 0x6470 + mask, "u64")
        check(ls, torch_gpu, x, False, "u64")


@pytest.mark.parametrize("kind,descending", [("u64", True), ("i64", False), ("i64", True), ("f64", False), ("f64", True)])
def test_digit_masks_other_kinds(ls, torch_gpu, kind, descending):
    """A dozen sets, among them {}, {0}, {7}, {0, 7}, {3, 4} and all eight bytes, descending and with
    int64 / float64 keys, on both paths, with and without positions."""
    C = ls.sort64_chunk_keys()
    for mask in DOZEN:
        for shape in ((1, 2 * C + 1), (3, 1000)):
            x = M.rows_with_bytes(shape, mask, 0x6480 + mask, kind)
            assert M.active_bytes(x, kind, descending) == mask
            check(ls, torch_gpu, x, descending, kind, with_idx=(mask & 2) == 0)


@KINDS
@pytest.mark.parametrize("which", ["1000", "C+1"])
def test_ties(ls, torch_gpu, which, kind):
    """Keys % 3 and all-equal keys: equal keys keep position order in both directions."""
    cols = cols_of(ls, which)
    x3 = M.generate("ties", (2, cols), 0x6490, kind)
    one = np.full((2, cols), M.specials(kind)[5], dtype=np.uint64)  # (float64: a NaN, so every key comes back changed)
    for x in (x3, one):
        for desc in BOTH:
            gk, gi = check(ls, torch_gpu, x, desc, kind)
            u = M.u_of(np.take_along_axis(x, gi.astype(np.int64), axis=1), kind, desc)
            assert bool((u[:, 1:] >= u[:, :-1]).all())
            tie = u[:, 1:] == u[:, :-1]
            assert bool((np.diff(gi.astype(np.int64), axis=1)[tie] > 0).all()), "equal keys out of position order"
    np.testing.assert_array_equal(gi, np.broadcast_to(np.arange(cols, dtype=np.uint32), (2, cols)))


@KINDS
def test_specials(ls, torch_gpu, kind):
    """A row of C + 1 keys with the kind's special values scattered through it: float64 NaNs of mixed
    sign and payload, +-0.0, +-inf and denormals (every NaN comes back as 0x7FFFFFFFFFFFFFFF); int64
    min, max, -1, 0 and 1; uint64 values across 2^63."""
    C = ls.sort64_chunk_keys()
    x = M.planted((2, C + 1), 0x64A0, kind)
    s = M.specials(kind)
    assert all(int((x == w).sum()) >= 2 for w in s)
    for desc in BOTH:
        gk, gi = check(ls, torch_gpu, x, desc, kind)
        if kind == "f64":
            nan = M.is_nan(gk)
            assert int(nan.sum()) == int(M.is_nan(x).sum()) >= 12
            assert bool((gk[nan] == np.uint64(M.NAN_OUT)).all())
            r = nan[:, ::-1] if desc else nan
            assert bool((np.diff(r.astype(np.int8), axis=1) >= 0).all()), "NaNs are the largest keys"
            ok = ~M.is_nan(x)
            np.testing.assert_array_equal(np.sort(gk[~nan]), np.sort(x[ok]))  # non-NaN keys bit-exact
    if kind != "f64":
        v = gk.view({"u64": np.uint64, "i64": np.int64}[kind])
        assert bool((v[:, 1:] <= v[:, :-1]).all())  # (the last call was descending)


@KINDS
@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1)])
def test_alignment(ls, torch_gpu, in_off, out_off, kind):
    """Input and output views that start one element (8 bytes) into a 256-byte aligned buffer, with odd
    cols, so that consecutive rows start on either 16-byte phase; both paths."""
    C = ls.sort64_chunk_keys()
    for rows, cols in ((3, 999), (3, C + 1), (2, 2 * C + 1)):
        x, exp = M.case(kind, rows, cols)
        check(ls, torch_gpu, x, in_off == 1, kind, exp=exp[in_off == 1], in_off=in_off, out_off=out_off)
    check(ls, torch_gpu, x, False, kind, exp=exp[False], with_idx=False, in_off=in_off, out_off=out_off)


def test_one_workspace_reused(ls, torch_gpu):
    """A sequence of calls that mix key types, directions, shapes, with and without positions and both
    paths on one workspace filled with 0xFF once and never cleared between them."""
    torch = torch_gpu
    C = ls.sort64_chunk_keys()
    seq = [("u64", 5, 300, True), ("f64", 2, 2 * C + 1, True), ("i64", 2, C, True), ("u64", 2, 2 * C + 1, False),
           ("f64", 3, 1000, False), ("i64", 3, C + 1, True), ("u64", 1, 3 * C - 1, True), ("f64", 3, C + 1, False),
           ("i64", 1, 65, True), ("f64", 1, 2 * C, True)]
    size = max(ls.sort64_workspace_bytes(r, c, True) for _, r, c, _ in seq)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (kind, rows, cols, with_idx) in enumerate(seq):
        x, exp = M.case(kind, rows, cols)
        desc = bool(i & 1) ^ (i >= 6)
        check(ls, torch, x, desc, kind, exp=exp[desc], with_idx=with_idx, ws=ws)


def test_graph_replay(ls, torch_gpu):
    """(1, 2C + 1) u64 with positions captured once on a side stream and replayed on keys whose images
    vary in 3, then 4, then 0 bytes (the last pass lands in the outputs from either side of the
    ping-pong, then no pass runs at all), then all 8: the plan is decided again on the device at every
    replay.  The launch sequence is linear."""
    torch = torch_gpu
    C = ls.sort64_chunk_keys()
    rows, cols = 1, 2 * C + 1
    src = torch.zeros((rows, cols), dtype=torch.int64, device="cuda")
    ko = torch.zeros((rows, cols), dtype=torch.int64, device="cuda")
    io = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sort64_workspace_bytes(rows, cols, True),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.sort64_device(src, rows, cols, ko, io, key="u64", workspace=ws, stream=s)
    s.synchronize()
    assert ls.sort64_passes(ws) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.sort64_device(src, rows, cols, ko, io, key="u64", workspace=ws, stream=torch.cuda.current_stream())
    for mask in (0b00010101, 0b11000011, 0, 0xFF, 0b00100000):
        x = M.rows_with_bytes((rows, cols), mask, 0x64B0 + mask, "u64")
        src.copy_(torch.from_numpy(x.view(np.int64)))
        ko.fill_(-1)
        io.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.sort64_workspace_status(ws)
        assert ls.sort64_passes(ws) == mask
        ek, ei = M.expected(x, False, "u64")
        np.testing.assert_array_equal(ko.cpu().numpy().view(np.uint64), ek, err_msg=f"keys, set {mask:#x}")
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=f"positions, set {mask:#x}")


@pytest.mark.parametrize("seed", [0x64C1, 0x64C2, 0x64C3, 0x64C4])
def test_seeded_sweep(ls, torch_gpu, seed):
    """40 cases, 10 per seed (sort64_model.sweep_cases): 1 to 5 rows of up to 3C keys, key type,
    direction, positions and generator drawn per case.  One workspace per seed, filled with 0xFF once."""
    torch = torch_gpu
    C = ls.sort64_chunk_keys()
    cases = list(M.sweep_cases(seed, C, count=10))
    size = max(ls.sort64_workspace_bytes(c["rows"], c["cols"], True) for c in cases)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    failures = []
    for i, c in enumerate(cases):
        try:
            check(ls, torch, c["x"], c["descending"], c["kind"], with_idx=c["with_idx"], ws=ws)
        except AssertionError as err:
            failures.append(f"seed {seed:#x} case {i}: {c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {seed:#x}: {[c['tag'] for c in cases]}")
    assert not failures, failures


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_sort_and_argsort(ls, torch_gpu, dtype):
    """ls.sort / ls.argsort of CUDA tensors against torch.sort(x, dim=-1, descending=d, stable=True) on
    NaN-free data without zeros of both signs: values, and indices after .int().  uint64, where torch
    has it, against the model (torch does not sort it)."""
    torch = torch_gpu
    C = ls.sort64_chunk_keys()
    g = torch.Generator().manual_seed(0x64D0)
    for shape in ((3, 1000), (2, 2 * C + 1), (2 * C + 5,), (77,)):
        if dtype == "float64":
            x = torch.randn(shape, generator=g, dtype=torch.float64)
            x.view(-1)[::7] = x.view(-1)[3]  # ties
        else:
            x = torch.randint(-(1 << 62), 1 << 62, shape, generator=g, dtype=torch.int64)
            x.view(-1)[::2] %= 1000
        xw = x.numpy().view(np.uint64).reshape(-1, shape[-1])
        if dtype == "uint64":
            x = x.view(torch.uint64)
        tg = x.cuda()
        keep = tg.clone()
        for desc in BOTH:
            v, i = ls.sort(tg, descending=desc)
            assert v.dtype == tg.dtype and i.dtype == torch.int32 and v.shape == tg.shape and i.shape == tg.shape
            a = ls.argsort(tg, descending=desc)
            assert a.dtype == torch.int32 and torch.equal(a, i)
            if dtype == "uint64":
                ek, ei = M.expected(xw, desc, "u64")
                np.testing.assert_array_equal(v.cpu().view(torch.int64).numpy().view(np.uint64).reshape(ek.shape), ek)
                np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32).reshape(ei.shape), ei)
            else:
                tv, ti = torch.sort(tg, dim=-1, descending=desc, stable=True)
                assert torch.equal(v, tv), f"values {dtype} {shape} descending={desc}"
                assert torch.equal(i, ti.int()), f"indices {dtype} {shape} descending={desc}"
        assert torch.equal(tg.view(torch.int64), keep.view(torch.int64)), "the input was written"
