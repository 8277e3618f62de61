"""labsort_topk_mask_device on the GPU: every row with all but its k best keys replaced by the fill,
and the mask of the keys kept, against the numpy model of the contract (tests/topk_mask_model.py), for
all five key types, at the smallest shapes at which the two paths -- one workgroup per row up to
C = kth_row_keys() keys, the select's launches and one streaming pass over chunks of C keys above --
can go wrong.  Every output asked for compares bit for bit (a NaN only has to be a NaN), every row's
mask sums to its k.  Every call runs on a workspace filled with 0xFF unless it is given one, on
outputs between guard elements that must keep their pattern, is followed by the status call, and out of
place must leave its input as it was."""
import numpy as np
import pytest

import kth_model as K
import rowsort_model as R
import sort_sweep_model as S
import topk_mask_model as TM
import topk_model as T

pytestmark = pytest.mark.gpu

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", R.KINDS)
FLOATS = ("f32", "bf16", "f16")
KPAT, MPAT, GUARD = 0x5A5A, 0x77, 8
C = T.constants()["TK_CHUNK"]


def sdtype(torch, kind):
    """The storage the words travel in: the library takes addresses."""
    return torch.int16 if R.is16(kind) else torch.int32


def to_dev(torch, x, kind):
    sd = np.int16 if R.is16(kind) else np.int32
    return torch.from_numpy(np.array(x).view(sd))  # (a writable copy: a shared case is read-only)


def k_arg(torch, k, rows):
    if isinstance(k, (int, np.integer)):
        return int(k)
    karg = torch.from_numpy((np.asarray(k, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
    assert karg.shape == (rows,)
    return karg


def run(ls, torch, x, k, largest, kind, fill=None, keys=True, mask=True, inplace=False, in_off=0, out_off=None,
        mask_off=0, ws=None, status=0):
    """in_off / out_off / mask_off: elements (bytes for the mask) between an aligned address and the
    matrix; out_off defaults to in_off, the phase at which whole groups go out as 16-byte stores.
    Returns (filtered words or None, mask bytes or None)."""
    rows, cols = x.shape
    n = rows * cols
    sd = sdtype(torch, kind)
    fill = TM.default_fill(kind, largest) if fill is None else fill
    store = torch.full((GUARD + in_off + n + GUARD,), 0x1111, dtype=sd, device="cuda")
    d = store[GUARD + in_off:GUARD + in_off + n]
    d.copy_(to_dev(torch, x, kind).reshape(-1))
    before = store.clone()
    out_off = in_off if out_off is None else out_off
    ostore = torch.full((GUARD + out_off + n + GUARD,), KPAT, dtype=sd, device="cuda")
    ko = (d if inplace else ostore[GUARD + out_off:GUARD + out_off + n]) if keys else None
    mstore = torch.full((GUARD + mask_off + n + GUARD,), MPAT, dtype=torch.uint8, device="cuda")
    mo = mstore[GUARD + mask_off:GUARD + mask_off + n] if mask else None
    if ws is None:
        ws = torch.full((ls.topk_mask_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    karg = k_arg(torch, k, rows)
    kbefore = None if isinstance(karg, int) else karg.clone()
    ls.topk_mask_device(d, rows, cols, karg, ko, mo, largest=largest, fill_bits=fill, key=kind, workspace=ws)
    assert ls.lib.labsort_topk_mask_workspace_status(ws.data_ptr(), None) == status
    assert kbefore is None or torch.equal(karg, kbefore), "d_k was written"
    lo, hi = GUARD + in_off, GUARD + in_off + n
    assert torch.equal(store[:lo], before[:lo]) and torch.equal(store[hi:], before[hi:]), "written outside the matrix"
    if not (keys and inplace):
        assert torch.equal(store, before), "the input was written"
    lo, hi = GUARD + out_off, GUARD + out_off + n
    assert bool((ostore[:lo] == KPAT).all()) and bool((ostore[hi:] == KPAT).all()), "written outside the key output"
    if not keys or inplace:
        assert bool((ostore == KPAT).all()), "keys were written without d_keys_out"
    lo, hi = GUARD + mask_off, GUARD + mask_off + n
    assert bool((mstore[:lo] == MPAT).all()) and bool((mstore[hi:] == MPAT).all()), "written outside the mask"
    if not mask:
        assert bool((mstore == MPAT).all()), "a mask byte was written without d_mask_out"
    gk = ko.cpu().numpy().view(R.wdtype(kind)).reshape(rows, cols) if keys else None
    gm = mo.cpu().numpy().reshape(rows, cols) if mask else None
    return gk, gm


def model(x, k, largest, kind, fill=None, exp=None):
    """exp: (keys, positions) of the rows sorted (rowsort_model.expected), when a test has them
    already: the first k positions; else the threshold form, O(cols) per row."""
    fill = TM.default_fill(kind, largest) if fill is None else fill
    if exp is None:
        return TM.by_threshold(x, k, largest, kind, fill)
    rows, cols = x.shape
    ks = K.ks_of(k, rows)
    m = np.zeros((rows, cols), dtype=np.uint8)
    for r in range(rows):
        m[r, exp[1][r, :int(ks[r])].astype(np.int64)] = 1
    return np.where(m != 0, x, R.wdtype(kind)(fill)).astype(x.dtype), m


def check(ls, torch, x, k, largest, kind, fill=None, exp=None, want=None, **kw):
    """want: the model's (words, mask) when the test computed it already.  k inside [1, cols]."""
    ek, em = want if want is not None else model(x, k, largest, kind, fill, exp)
    np.testing.assert_array_equal(em.sum(axis=1), K.ks_of(k, x.shape[0]))
    gk, gm = run(ls, torch, x, k, largest, kind, fill=fill, **kw)
    TM.assert_result(gk, gm, ek, em, kind, f"{kind} {x.shape} k={k} largest={largest} {kw}")
    return gk, gm


def test_shapes(ls):
    assert ls.kth_row_keys() == C == 16384


@KINDS
@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 1000, 4096, 4097, C])
def test_short_rows(ls, torch_gpu, cols, kind):
    """4096 / 4097: the last row of the 256-thread workgroup and the first of the 1024-thread one; C:
    the longest row one workgroup holds, on the 256-byte workspace."""
    assert ls.topk_mask_workspace_bytes(5, cols) == 256
    x, exp = R.case(kind, 3 if cols == C else 5, cols)
    for largest in BOTH:
        for k in sorted({1, (cols + 1) // 2, cols}):
            check(ls, torch_gpu, x, k, largest, kind, exp=exp[largest])


@KINDS
@pytest.mark.parametrize("which", ["C+1", "2C", "2C+1", "3C-1"])
def test_path_and_chunk_edges(ls, torch_gpu, which, kind):
    """C + 1: the first long row, whose last chunk holds one key."""
    cols = {"C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1}[which]
    assert ls.topk_mask_workspace_bytes(2, cols) > 256
    x3, exp3 = R.case(kind, 3, cols)
    x = x3[:2]
    for largest in BOTH:
        exp = (exp3[largest][0][:2], exp3[largest][1][:2])
        for k in (1, C, cols // 2 + 1, cols):
            check(ls, torch_gpu, x, k, largest, kind, exp=exp)


def tie_row(kind, largest):
    """A row of 3C - 1 random keys in which one key occurs at eight chosen positions and nowhere else:
    three in chunk 0, three in chunk 1, two in chunk 2.  Returns the row, the positions and the number
    of keys in front of the ties."""
    cols = 3 * C - 1
    row = R.random_words((cols,), 0x7A31, kind)
    at = np.array([5, 100, C - 1, C, C + 77, 2 * C - 1, 2 * C, 3 * C - 2])
    u = R.u_of(row.reshape(1, -1), kind, largest)[0]
    t = row[int(np.argsort(u, kind="stable")[cols // 2])]  # (a middle key: never a NaN)
    other = row[int(np.argsort(u, kind="stable")[cols // 2 + 1000])]
    assert R.u_of(np.array([[t]]), kind, largest)[0, 0] != R.u_of(np.array([[other]]), kind, largest)[0, 0]
    row[row == t] = other
    row[at] = t
    u = R.u_of(row.reshape(1, -1), kind, largest)[0]
    ut = R.u_of(np.array([[t]], dtype=row.dtype), kind, largest)[0, 0]
    assert np.flatnonzero(u == ut).tolist() == at.tolist()
    return row, at, int(np.count_nonzero(u < ut))


@KINDS
def test_ties_across_chunks(ls, torch_gpu, kind):
    """k cuts at the first tie, at the last tie of chunk 0, at the first of chunk 1, inside chunk 1 and
    at the very last tie: the ties in front of the cut are kept, those behind it are not."""
    for largest in BOTH:
        row, at, below = tie_row(kind, largest)
        cuts = [1, 3, 4, 5, 8]
        x = np.ascontiguousarray(np.broadcast_to(row, (len(cuts), row.size)))
        ks = below + np.array(cuts)
        gk, gm = check(ls, torch_gpu, x, ks, largest, kind)
        for r, c in enumerate(cuts):
            assert gm[r, at].tolist() == [1] * c + [0] * (8 - c)
        check(ls, torch_gpu, x[:1], int(ks[3]), largest, kind, keys=False)


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16"])
@pytest.mark.parametrize("cols", [65, 4096, 4097, C])
def test_select_and_filter_agree(ls, torch_gpu, cols, kind):
    """Short rows, where kth_device and topk_mask_device run one kernel template: the two calls
    against each other, no model between them.  Half of the keys take one of four values, so the
    threshold has many ties.  With (T, P) what the select returns for a row: the mask has k ones,
    the last kept tie of T sits at P, and no kept key is worse than T."""
    torch = torch_gpu
    rows = 3
    rng = np.random.default_rng(0x7A50 + cols)
    x = R.random_words((rows, cols), 0x7A51 + cols, kind)
    four = x[0, :4].copy()
    tied = rng.random((rows, cols)) < 0.5
    x[tied] = four[rng.integers(0, 4, size=int(tied.sum()))]
    d = to_dev(torch, x, kind).cuda()
    for largest in BOTH:
        u = R.u_of(x, kind, largest)
        for k in sorted({1, cols // 2, cols}):
            ko = torch.empty(rows, dtype=sdtype(torch, kind), device="cuda")
            io = torch.empty(rows, dtype=torch.int32, device="cuda")
            ls.kth_device(d, rows, cols, k, ko, io, largest=largest, key=kind)
            uT = R.u_of(ko.cpu().numpy().view(R.wdtype(kind)).reshape(rows, 1), kind, largest)[:, 0]
            P = io.cpu().numpy().view(np.uint32)
            _, gm = run(ls, torch, x, k, largest, kind)
            for r in range(rows):
                msg = f"{kind} cols={cols} k={k} largest={largest} row {r}"
                assert int(gm[r].sum()) == k, msg
                assert int(np.flatnonzero((u[r] == uT[r]) & (gm[r] != 0))[-1]) == int(P[r]), msg
                assert int(u[r][gm[r] != 0].max()) <= int(uT[r]), msg


@KINDS
@pytest.mark.parametrize("cols", [1000, 3 * C - 1])
def test_all_equal_rows(ls, torch_gpu, cols, kind):
    word = R.random_words((1,), 0x7A32, kind)[0]
    x = np.full((2, cols), word, dtype=R.wdtype(kind))
    for largest in BOTH:
        for k in (1, cols // 2, cols):
            gk, gm = check(ls, torch_gpu, x, k, largest, kind)
            assert bool((gm[:, :k] == 1).all()) and bool((gm[:, k:] == 0).all())


@pytest.mark.parametrize("kind", FLOATS)
@pytest.mark.parametrize("cols", [1000, 2 * C + 1])
def test_all_nan_rows(ls, torch_gpu, cols, kind):
    """NaNs of several payloads and both signs are one value: the first k positions are kept and come
    back as the canonical NaN."""
    x = S.sweep_row("all_nan", cols, kind, False, np.random.default_rng(0x7A33)).reshape(1, cols).astype(R.wdtype(kind))
    x = np.ascontiguousarray(np.broadcast_to(x, (2, cols)))
    canon = 0x7FFF if R.is16(kind) else 0x7FFFFFFF
    for largest in BOTH:
        for k in (1, cols // 3, cols):
            gk, gm = check(ls, torch_gpu, x, k, largest, kind, fill=0)
            assert bool((gm[:, :k] == 1).all()) and bool((gm[:, k:] == 0).all())
            assert bool((gk[:, :k] == canon).all()) and bool((gk[:, k:] == 0).all())


@pytest.mark.parametrize("kind", FLOATS)
@pytest.mark.parametrize("cols", [300, C + 1])
def test_nans_and_zeros_straddle_the_cut(ls, torch_gpu, cols, kind):
    """Four NaNs of different payloads among finite keys: the largest two keys are the first two NaNs
    by position, the smallest cols - 2 leave out the last two.  Three -0.0 and three +0.0 among keys
    that are all above zero (largest=False) cut between the zeros: the negative ones go first; with
    largest=True and all other keys below zero the positive ones do."""
    is16 = R.is16(kind)
    one = {"f32": 0x3F800000, "bf16": 0x3F80, "f16": 0x3C00}[kind]
    sign = 0x8000 if is16 else 0x80000000
    wd = R.wdtype(kind)
    rng = np.random.default_rng(0x7A34)
    base = (one + rng.integers(1, 100, size=cols)).astype(wd)  # finite keys above 1.0
    nans = [R.nan_word(kind), (0x7FC1 if is16 else 0x7FC00001), (0xFFFF if is16 else 0xFFFFFFFF), (0x7FFF if is16 else 0x7FFFFFFF)]
    at = np.array([3, cols // 2, cols // 2 + 1, cols - 1])
    x = base.copy()
    x[at] = np.array(nans, dtype=wd)
    x = x.reshape(1, cols)
    gk, gm = check(ls, torch_gpu, x, 2, True, kind)
    assert np.flatnonzero(gm[0]).tolist() == at[:2].tolist()
    gk, gm = check(ls, torch_gpu, x, cols - 2, False, kind)
    assert np.flatnonzero(gm[0] == 0).tolist() == at[2:].tolist()
    zat = np.array([1, 2, cols // 2, cols // 2 + 2, cols - 3, cols - 2])
    zs = np.array([0, sign, sign, 0, 0, sign], dtype=wd)
    x = base.copy()
    x[zat] = zs
    gk, gm = check(ls, torch_gpu, x.reshape(1, cols), 4, False, kind)  # the three -0.0 and the first +0.0
    assert np.flatnonzero(gm[0]).tolist() == [1, 2, cols // 2, cols - 2]
    x = (base | wd(sign)).astype(wd)  # all below -1.0
    x[zat] = zs
    gk, gm = check(ls, torch_gpu, x.reshape(1, cols), 4, True, kind)  # the three +0.0 and the first -0.0
    assert np.flatnonzero(gm[0]).tolist() == [1, 2, cols // 2 + 2, cols - 3]


@KINDS
def test_fill_equals_a_key(ls, torch_gpu, kind):
    """The fill is data: a fill that is a key of the row, kept or not, changes the keys output only
    where the mask is 0."""
    for rows, cols in ((3, 1000), (2, 2 * C + 1)):
        x, exp = R.case(kind, rows, cols, "random")
        for largest in BOTH:
            for fill in (int(exp[largest][0][0, 0]), int(exp[largest][0][0, cols - 1])):  # row 0's best and worst key
                gk, gm = check(ls, torch_gpu, x, cols // 2, largest, kind, fill=fill, exp=exp[largest])
                assert bool((gk[gm == 0] == fill).all())


@KINDS
def test_per_row_k(ls, torch_gpu, kind):
    """7 rows of 2C + 1 with seven different k; then one row's k set to 0 and another's to cols + 1:
    the status call reports ERR_ARG, the other rows are right, the two rows are filtered with the
    clamped k, the guards are intact.  The same on the one-launch path."""
    x, exp = R.case(kind, 7, 2 * C + 1)
    cols = x.shape[1]
    ks = np.array([1, cols, 2, cols // 2, C, C + 1, cols - 1])
    for largest in BOTH:
        check(ls, torch_gpu, x, ks, largest, kind, exp=exp[largest])
        bad = ks.copy()
        bad[2], bad[5] = 0, cols + 1
        clamped, which = K.clamp(bad, cols)
        assert which.tolist() == [False, False, True, False, False, True, False]
        ek, em = model(x, clamped, largest, kind, exp=exp[largest])
        gk, gm = run(ls, torch_gpu, x, bad, largest, kind, status=ls.ERR_ARG)
        TM.assert_result(gk, gm, ek, em, kind, "clamped k")
        assert gm.sum(axis=1).tolist() == clamped.tolist()
    x, exp = R.case(kind, 5, 1000)
    bad = np.array([1, -1, 500, 0, 1000])
    clamped = K.clamp(bad, 1000)[0]
    ek, em = model(x, clamped, False, kind, exp=exp[False])
    gk, gm = run(ls, torch_gpu, x, bad, False, kind, status=ls.ERR_ARG)
    TM.assert_result(gk, gm, ek, em, kind, "clamped k, short rows")
    check(ls, torch_gpu, x, np.array([1, 7, 500, 999, 1000]), True, kind, exp=exp[True])


@KINDS
def test_output_combinations(ls, torch_gpu, kind):
    """Keys only, mask only and both give the same keys and the same mask, and an output that is not
    asked for is not written (run() checks its whole storage), on both paths."""
    for rows, cols in ((3, 4097), (2, 2 * C + 1)):
        x, exp = R.case(kind, rows, cols)
        for largest in BOTH:
            want = model(x, cols // 3, largest, kind, exp=exp[largest])
            for keys, mask in ((True, True), (True, False), (False, True)):
                check(ls, torch_gpu, x, cols // 3, largest, kind, want=want, keys=keys, mask=mask)


def test_one_workspace_reused(ls, torch_gpu):
    """Calls that mix key types, directions, paths, shapes and outputs on one workspace, never cleared
    between them; a call with a bad k in between does not leak into the next one's status."""
    torch = torch_gpu
    seq = [("bf16", 3, 2 * C + 1), ("i32", 5, 1000), ("f32", 3, 2 * C + 1), ("f16", 3, C + 1), ("u32", 3, 3 * C - 1),
           ("bf16", 3, 4097), ("f32", 3, C)]
    ws = torch.full((max(ls.topk_mask_workspace_bytes(r, c) for _, r, c in seq),), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (kind, rows, cols) in enumerate(seq):
        x, exp = R.case(kind, rows, cols)
        largest = bool(i & 1)
        if i == 2:
            run(ls, torch, x, np.array([0, 5, cols]), largest, kind, ws=ws, status=ls.ERR_ARG)
        check(ls, torch, x, cols // 2, largest, kind, exp=exp[largest], ws=ws, mask=i != 4, inplace=i == 3)
        check(ls, torch, x, np.arange(1, rows + 1) * (cols // rows), not largest, kind, exp=exp[not largest], ws=ws, keys=i != 5)


@KINDS
def test_in_place(ls, torch_gpu, kind):
    """d_keys_out == d_keys, short and long rows: what the out-of-place call gives."""
    for rows, cols in ((5, 1000), (3, 4097), (3, C), (2, C + 1), (3, 3 * C - 1)):
        x, exp = R.case(kind, rows, cols)
        for largest in BOTH:
            for k in (cols // 2 + 1, np.arange(1, rows + 1) * (cols // rows)):
                want = model(x, k, largest, kind, exp=exp[largest])
                ok, om = check(ls, torch_gpu, x, k, largest, kind, want=want)
                ik, im = check(ls, torch_gpu, x, k, largest, kind, want=want, inplace=True)
                np.testing.assert_array_equal(ik, ok)
                np.testing.assert_array_equal(im, om)
            check(ls, torch_gpu, x, 7, largest, kind, exp=exp[largest], inplace=True, mask=False)


PHASE_ROWS = 9  # odd rows of odd length: every row starts at another phase, the neighbours run at the same time


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("cols", [63, 4097, 2 * C + 1])
def test_16bit_phases(ls, torch_gpu, cols, kind):
    """Rows of odd length share their first and last 4 and 16 bytes with their neighbours.  The input
    0 .. 7 elements into its 16 bytes; the keys output at the same phase (16-byte stores), at another
    (element stores) and in place."""
    x = R.planted_words((PHASE_ROWS, cols), 0x7A35 + cols, kind)
    x[::3] = R.tie_words((PHASE_ROWS, cols), 0x7A36 + cols, kind)[::3]
    ks = np.random.default_rng(0x7A37).integers(1, cols + 1, size=PHASE_ROWS)
    want = model(x, ks, True, kind)
    for in_off in range(8):
        check(ls, torch_gpu, x, ks, True, kind, want=want, in_off=in_off, mask_off=(3 * in_off + 1) % 8)
        check(ls, torch_gpu, x, ks, True, kind, want=want, in_off=in_off, out_off=(in_off + 3) % 8, mask=False)
        check(ls, torch_gpu, x, ks, True, kind, want=want, in_off=in_off, inplace=True, mask=in_off % 2 == 0)


@pytest.mark.parametrize("kind", ["u32", "i32", "f32"])
@pytest.mark.parametrize("cols", [63, 4097, 2 * C + 1])
def test_32bit_phases(ls, torch_gpu, cols, kind):
    x = R.planted_words((PHASE_ROWS, cols), 0x7A38 + cols, kind)
    ks = np.random.default_rng(0x7A39).integers(1, cols + 1, size=PHASE_ROWS)
    want = model(x, ks, False, kind)
    for in_off in range(4):
        check(ls, torch_gpu, x, ks, False, kind, want=want, in_off=in_off, mask_off=(3 * in_off + 1) % 8)
        check(ls, torch_gpu, x, ks, False, kind, want=want, in_off=in_off, out_off=(in_off + 1) % 4, mask=False)
        check(ls, torch_gpu, x, ks, False, kind, want=want, in_off=in_off, inplace=True, mask=in_off % 2 == 0)


@pytest.mark.parametrize("kind", ["i32", "bf16"])
@pytest.mark.parametrize("cols", [63, 64, 4097, 2 * C + 1])
def test_mask_phases(ls, torch_gpu, cols, kind):
    """The mask 0 .. 7 bytes into its 8 bytes, whatever the keys' phase; mask only and with keys."""
    x = R.planted_words((PHASE_ROWS, cols), 0x7A3A + cols, kind)
    ks = np.random.default_rng(0x7A3B).integers(1, cols + 1, size=PHASE_ROWS)
    want = model(x, ks, True, kind)
    for mask_off in range(8):
        check(ls, torch_gpu, x, ks, True, kind, want=want, mask_off=mask_off, keys=mask_off % 2 == 1, in_off=mask_off // 2)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("cols", [4097, 2 * C + 1])
def test_graph_replay(ls, torch_gpu, cols, kind):
    """A call with d_k captured once on a side stream and replayed on new keys and new k values in the
    same buffers.  The launch sequence is linear."""
    torch = torch_gpu
    rows = 3
    sd = sdtype(torch, kind)
    src = torch.zeros((rows, cols), dtype=sd, device="cuda")
    dk = torch.ones((rows,), dtype=torch.int32, device="cuda")
    ko = torch.zeros((rows, cols), dtype=sd, device="cuda")
    mo = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    ws = torch.full((ls.topk_mask_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    fill = TM.default_fill(kind, True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.topk_mask_device(src, rows, cols, dk, ko, mo, largest=True, fill_bits=fill, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.topk_mask_device(src, rows, cols, dk, ko, mo, largest=True, fill_bits=fill, key=kind, workspace=ws,
                            stream=torch.cuda.current_stream())
    inputs = {"random": R.random_words((rows, cols), 0x7A3C, kind), "ties": R.tie_words((rows, cols), 0x7A3D, kind),
              "planted": R.planted_words((rows, cols), 0x7A3E, kind)}
    rng = np.random.default_rng(0x7A3F)
    for dist, x in inputs.items():
        x = np.ascontiguousarray(x, dtype=R.wdtype(kind))
        ks = rng.integers(1, cols + 1, size=rows)
        src.copy_(to_dev(torch, x, kind))
        dk.copy_(torch.from_numpy(ks.astype(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.topk_mask_workspace_status(ws)
        ek, em = TM.by_threshold(x, ks, True, kind, fill)
        TM.assert_result(ko.cpu().numpy().view(R.wdtype(kind)), mo.cpu().numpy(), ek, em, kind, dist)


SWEEP_SEED = 131
SWEEP_CASES = 40


def sweep_cases(seed):
    """SWEEP_CASES cases: cols log-uniform in [1, 3C], a third of the cases on m C + {-1, 0, 1}; 1 .. 6
    rows; every kind; every row from its own generator (sort_sweep_model.sweep_row); direction, the
    outputs, in place and the phases random; half of the cases with a random k per row."""
    for i in range(SWEEP_CASES):
        rng = np.random.default_rng([seed, 0x7A7A, i])
        if i % 3 == 0:
            cols = min(max(int(rng.integers(1, 4)) * C + int(rng.integers(-1, 2)), 1), 3 * C)
        else:
            cols = min(max(int(np.exp(rng.uniform(0.0, np.log(3 * C)))), 1), 3 * C)
        rows = int(rng.integers(1, 7))
        kind = R.KINDS[int(rng.integers(0, len(R.KINDS)))]
        largest = bool(rng.integers(0, 2))
        keys, mask = ((True, True), (True, False), (False, True))[int(rng.integers(0, 3))]
        inplace = keys and bool(rng.integers(0, 2))
        in_off, mask_off = int(rng.integers(0, 8 if R.is16(kind) else 4)), int(rng.integers(0, 8))
        gens = [S.pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([S.sweep_row(g, cols, kind, largest, rng) for g in gens]).astype(R.wdtype(kind))
        k = rng.integers(1, cols + 1, size=rows) if i % 2 else int(rng.integers(1, cols + 1))
        tag = f"seed={seed} case={i} {kind} ({rows}, {cols}) k={k} largest={largest} keys={keys} mask={mask} inplace={inplace} in_off={in_off} mask_off={mask_off} rows={gens}"
        yield dict(x=x, k=k, kind=kind, largest=largest, tag=tag,
                   kw=dict(keys=keys, mask=mask, inplace=inplace, in_off=in_off, mask_off=mask_off))


def test_seeded_sweep(ls, torch_gpu):
    """One workspace, filled with 0xFF once and never cleared between the cases."""
    torch = torch_gpu
    cases = list(sweep_cases(SWEEP_SEED))
    assert len(cases) == SWEEP_CASES
    ws = torch.full((max(ls.topk_mask_workspace_bytes(*c["x"].shape) for c in cases),), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths = [], {"short": 0, "long": 0}
    for c in cases:
        paths["short" if c["x"].shape[1] <= ls.kth_row_keys() else "long"] += 1
        try:
            check(ls, torch, c["x"], c["k"], c["largest"], c["kind"], ws=ws, **c["kw"])
        except AssertionError as err:
            failures.append(f"{c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {SWEEP_SEED}: {paths}")
    assert paths["short"] >= 5 and paths["long"] >= 5
    assert not failures, failures


def test_one_long_row(ls, torch_gpu):
    """One int32 row of 1024 C + C + 9 keys, mask only: 1025 chunks, so the histogram workgroups count
    two chunks each and the last pick's scan along the chunks takes a second step; ties of the
    threshold in the first and in the last chunk."""
    kind = "i32"
    cols = 1024 * C + C + 9
    x = R.random_words((1, cols), 0x7A40, kind)
    x[0, ::4099] = x[0, 7]
    x[0, -3:] = x[0, 7]
    below = int(np.count_nonzero(R.u_of(x, kind)[0] < R.u_of(x[:, 7:8], kind)[0, 0]))
    ties = int(np.count_nonzero(x[0] == x[0, 7]))
    check(ls, torch_gpu, x, below + ties - 2, False, kind, keys=False)


def tie_free(torch, rows, cols, kind, seed):
    """A tensor of distinct finite nonzero keys per row (int32: distinct integers)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "i32":
        return torch.stack([torch.randperm(cols, generator=g) - cols // 2 for _ in range(rows)]).to(torch.int32).cuda()
    if kind == "f32":
        return torch.stack([(torch.randperm(cols, generator=g) - cols // 2).to(torch.float32) + 0.5 for _ in range(rows)]).cuda()
    top = 0x7F7F if kind == "bf16" else 0x7BFF  # the largest finite pattern
    pats = torch.cat([torch.arange(1, top + 1), torch.arange(0x8001, 0x8000 + top + 1)])
    assert cols <= pats.numel()
    x = torch.stack([pats[torch.randperm(pats.numel(), generator=g)[:cols]] for _ in range(rows)])
    x = torch.where(x >= 0x8000, x - 0x10000, x).to(torch.int16)
    return x.cuda().view(torch.bfloat16 if kind == "bf16" else torch.float16)


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16", "f16"])
def test_python_topk_filter_and_mask(ls, torch_gpu, kind):
    """ls.topk_filter and ls.topk_mask against torch.topk's indices scattered onto a filled tensor, on
    rows without ties: an int k and a tensor k, both directions, the default and a given fill, out=None,
    another tensor and x itself, a 1-D tensor; and the TypeErrors that need a CUDA x."""
    torch = torch_gpu
    for rows, cols in ((4, 1000), (3, 2 * C + 1)):
        x = tie_free(torch, rows, cols, kind, 0x7A41 + cols)
        kt = torch.tensor([1, cols // 2, cols, 77][:rows], dtype=torch.int32, device="cuda")
        for largest in BOTH:
            for k in (50, kt):
                ks = [k] * rows if isinstance(k, int) else kt.tolist()
                for fill in (None, 3):
                    if fill is None:
                        f = (torch.iinfo(torch.int32).min if largest else torch.iinfo(torch.int32).max) if kind == "i32" \
                            else (float("-inf") if largest else float("inf"))
                    else:
                        f = fill
                    ref = torch.full_like(x, f)
                    rmask = torch.zeros(x.shape, dtype=torch.bool, device="cuda")
                    for r in range(rows):
                        idx = torch.topk(x[r].float() if kind != "i32" else x[r], ks[r], largest=largest).indices
                        ref[r, idx] = x[r, idx]
                        rmask[r, idx] = True
                    got = ls.topk_filter(x, k, largest=largest, fill=fill)
                    assert got.dtype == x.dtype and got.shape == x.shape and got.data_ptr() != x.data_ptr()
                    assert torch.equal(got.view(sdtype(torch, kind)), ref.view(sdtype(torch, kind)))
                    out = torch.empty_like(x)
                    assert ls.topk_filter(x, k, largest=largest, fill=fill, out=out) is out
                    assert torch.equal(out.view(sdtype(torch, kind)), ref.view(sdtype(torch, kind)))
                    y = x.clone()
                    assert ls.topk_filter(y, k, largest=largest, fill=fill, out=y) is y
                    assert torch.equal(y.view(sdtype(torch, kind)), ref.view(sdtype(torch, kind)))
                m = ls.topk_mask(x, k, largest=largest)
                assert m.dtype == torch.bool and m.shape == x.shape and torch.equal(m, rmask)
        row = x[1].contiguous()  # 1-D: one row
        got = ls.topk_filter(row, 5)
        assert got.shape == row.shape and int(ls.topk_mask(row, 5).sum()) == 5
        assert torch.equal(got[ls.topk_mask(row, 5)].sort().values, torch.topk(row.float() if kind != "i32" else row, 5).values.sort().values.to(row.dtype))
        for badk in (kt.to(torch.int64), kt[:2], kt.cpu(), kt.view(1, -1), 2.5, "3", None, True):
            for f in (ls.topk_filter, ls.topk_mask):
                with pytest.raises(TypeError):
                    f(x, badk)
        for bad_out in (torch.empty_like(x).to(torch.float64), torch.empty((rows, cols + 1), dtype=x.dtype, device="cuda"),
                        torch.empty((cols, rows), dtype=x.dtype, device="cuda").t(), torch.empty(x.shape, dtype=x.dtype), "out"):
            with pytest.raises(TypeError):
                ls.topk_filter(x, 3, out=bad_out)
        with pytest.raises(ls.LabsortError):
            ls.topk_filter(x, cols + 1)  # the host k is checked before any launch
        with pytest.raises(ls.LabsortError) as e:
            ls.topk_mask(x, torch.zeros(rows, dtype=torch.int32, device="cuda"))  # a device k: reported by the status
        assert e.value.status == ls.ERR_ARG
