"""labsort_top_p_device on the GPU: every row reduced to the smallest prefix of its most probable
elements whose fixed-point mass reaches p, the mask of the elements kept and their number, against the
numpy model of the contract (tests/top_p_model.py) bit for bit (a NaN only has to be a NaN), and against
labsort_topk_mask_device run on the counts the call returned, byte for byte, for the three key types, at
the smallest shapes at which the two paths -- one workgroup per row up to C = kth_row_keys() keys, the
mass select's launches and the streaming pass over chunks of C keys above -- can go wrong.  Every call
runs on a workspace filled with 0xFF unless it is given one, on outputs between guard elements that
must keep their pattern, is followed by the status call, must leave d_p as it was and, out of place, its
input too."""
import numpy as np
import pytest

import rowsort_model as R
import sort_sweep_model as S
import top_p_model as P
import topk_model as T

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", P.KINDS)
KPAT, MPAT, CPAT, GUARD = 0x5A5A, 0x77, 0x5A5A5A5A, 8
C = T.constants()["TK_CHUNK"]
PS = (2.0 ** -30, 0.5, 0.9, 1.0)
ONE = {"f32": 0x3F800000, "bf16": 0x3F80, "f16": 0x3C00}


def sdtype(torch, kind):
    """The storage the words travel in: the library takes addresses."""
    return torch.int16 if R.is16(kind) else torch.int32


def to_dev(torch, x, kind):
    sd = np.int16 if R.is16(kind) else np.int32
    return torch.from_numpy(np.array(x).view(sd))  # (a writable copy)


def p_arg(torch, p, rows):
    if isinstance(p, (float, int)):
        return float(p)
    parg = torch.from_numpy(np.array(p, dtype=np.float32)).cuda()
    assert parg.shape == (rows,)
    return parg


def run(ls, torch, x, p, kind, fill=0, keys=True, mask=True, kept=True, inplace=False, in_off=0, out_off=None,
        mask_off=0, ws=None, status=0):
    """in_off / out_off / mask_off: elements (bytes for the mask) between an aligned address and the
    matrix; out_off defaults to in_off, the phase at which whole groups go out as 16-byte stores.
    Returns (filtered words or None, mask bytes or None, counts or None)."""
    rows, cols = x.shape
    n = rows * cols
    sd = sdtype(torch, kind)
    store = torch.full((GUARD + in_off + n + GUARD,), 0x1111, dtype=sd, device="cuda")
    d = store[GUARD + in_off:GUARD + in_off + n]
    d.copy_(to_dev(torch, x, kind).reshape(-1))
    before = store.clone()
    out_off = in_off if out_off is None else out_off
    ostore = torch.full((GUARD + out_off + n + GUARD,), KPAT, dtype=sd, device="cuda")
    ko = (d if inplace else ostore[GUARD + out_off:GUARD + out_off + n]) if keys else None
    mstore = torch.full((GUARD + mask_off + n + GUARD,), MPAT, dtype=torch.uint8, device="cuda")
    mo = mstore[GUARD + mask_off:GUARD + mask_off + n] if mask else None
    cstore = torch.full((GUARD + rows + GUARD,), CPAT, dtype=torch.int32, device="cuda")
    co = cstore[GUARD:GUARD + rows] if kept else None
    if ws is None:
        ws = torch.full((ls.top_p_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    parg = p_arg(torch, p, rows)
    pbefore = None if isinstance(parg, float) else parg.clone()
    ls.top_p_device(d, rows, cols, parg, ko, mo, co, fill_bits=fill, key=kind, workspace=ws)
    assert ls.lib.labsort_top_p_workspace_status(ws.data_ptr(), None) == status
    assert pbefore is None or torch.equal(parg.view(torch.int32), pbefore.view(torch.int32)), "d_p was written"
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
    assert bool((cstore[:GUARD] == CPAT).all()) and bool((cstore[GUARD + rows:] == CPAT).all()), "written outside the counts"
    if not kept:
        assert bool((cstore == CPAT).all()), "a count was written without d_kept_out"
    gk = ko.cpu().numpy().view(R.wdtype(kind)).reshape(rows, cols) if keys else None
    gm = mo.cpu().numpy().reshape(rows, cols) if mask else None
    gc = co.cpu().numpy().view(np.uint32).astype(np.int64) if kept else None
    return gk, gm, gc


def topk_mask_of(ls, torch, x, ks, kind, fill):
    """What labsort_topk_mask_device(largest = 1) gives with d_k = ks: (words, mask)."""
    rows, cols = x.shape
    d = to_dev(torch, x, kind).cuda()
    ko = torch.empty_like(d)
    mo = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    dk = torch.from_numpy(np.asarray(ks, dtype=np.int32)).cuda()
    ls.topk_mask_device(d, rows, cols, dk, ko, mo, largest=True, fill_bits=fill, key=kind)
    return ko.cpu().numpy().view(R.wdtype(kind)), mo.cpu().numpy()


def check(ls, torch, x, p, kind, fill=0, exp=None, want=None, cross=False, **kw):
    """want: the model's (words, mask, counts, flagged) when the test computed it already; exp: the rows
    sorted descending.  cross: also against topk_mask_device on the counts returned."""
    if want is None:
        want = P.by_scan(x, p, kind, fill, exp) if exp is not None else P.by_threshold(x, p, kind, fill)
    ek, em, ec, flagged = want
    np.testing.assert_array_equal(em.sum(axis=1), ec)
    gk, gm, gc = run(ls, torch, x, p, kind, fill=fill, status=ls.ERR_ARG if flagged else ls.OK, **kw)
    msg = f"{kind} {x.shape} p={p} {kw}"
    if gc is not None:
        np.testing.assert_array_equal(gc, ec, err_msg=f"counts {msg}")
    if gm is not None:
        np.testing.assert_array_equal(gm, em, err_msg=f"mask {msg}")
    if gk is not None:
        R.assert_keys(gk, ek, kind, msg)
    if cross:
        tk, tm = topk_mask_of(ls, torch, x, gc, kind, fill)
        np.testing.assert_array_equal(gk, tk, err_msg=f"keys against topk_mask_device {msg}")
        np.testing.assert_array_equal(gm, tm, err_msg=f"mask against topk_mask_device {msg}")
    return gk, gm, gc


def rows_p(rows, seed):
    """One p per row: random, the first 1.0, the second tiny."""
    p = np.random.default_rng(seed).random(rows).astype(np.float32)
    p[0] = 1.0
    if rows > 1:
        p[1] = 2.0 ** -30
    return np.maximum(p, np.float32(2.0 ** -32))


def test_shapes(ls):
    assert ls.kth_row_keys() == C == 16384


@KINDS
@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 1000, 4096, 4097, C])
def test_short_rows(ls, torch_gpu, cols, kind):
    """4096 / 4097: the last row of the 256-thread workgroup and the first of the 1024-thread one; C:
    the longest row one workgroup holds, on the 256-byte workspace.  Softmax rows, two of them with
    NaNs, values above 1, negatives, zeros, tiny values and a large tie block planted."""
    assert ls.top_p_workspace_bytes(5, cols) == 256
    x = P.special_rows(kind, cols, 0x70C0 + cols)[[0, 1, 3]]
    if cols != C:
        x = np.concatenate([x, P.softmax_words(cols, kind, 0x70C1 + cols, 0.7, rows=2)])
    exp = R.expected(x, True, kind)
    for p in PS + (rows_p(x.shape[0], 0x70C2 + cols),):
        check(ls, torch_gpu, x, p, kind, exp=exp, cross=True)


@KINDS
@pytest.mark.parametrize("which", ["C+1", "2C", "2C+1", "3C-1"])
def test_path_and_chunk_edges(ls, torch_gpu, which, kind):
    """C + 1: the first long row, whose last chunk holds one key."""
    cols = {"C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1}[which]
    assert ls.top_p_workspace_bytes(2, cols) > 256
    x = P.special_rows(kind, cols, 0x70C3 + cols)[[0, 3]]
    exp = R.expected(x, True, kind)
    for p in PS + (rows_p(2, 0x70C4 + cols),):
        check(ls, torch_gpu, x, p, kind, exp=exp, cross=True)


@KINDS
@pytest.mark.parametrize("cols", [1000, 2 * C + 1])
def test_all_equal_rows(ls, torch_gpu, cols, kind):
    """k = ceil(t / w) and the lowest positions are kept; at p = 1 the last tie kept is the single key
    of the last chunk."""
    word = P.words_of(np.array([1.0 / 1024]), kind)[0]
    w = int(P.weight(np.array([word]), kind)[0])
    assert w == P.ONE >> 10
    x = np.full((2, cols), word, dtype=R.wdtype(kind))
    for p in (2.0 ** -30, 0.3, 0.5, 1.0, np.array([0.7, 1.0], dtype=np.float32)):
        gk, gm, gc = check(ls, torch_gpu, x, p, kind, fill=3)
        for r in range(2):
            Pr = P.fixed_p(P.ps_of(p, 2)[r])[0]
            k = -(-P.target(Pr, cols * w) // w)
            assert gc[r] == k and bool((gm[r, :k] == 1).all()) and bool((gm[r, k:] == 0).all())
    assert gc[1] == cols


@KINDS
def test_tie_block_straddles_a_chunk_edge(ls, torch_gpu, kind):
    """Seven ties of 1/8 at C - 3 .. C + 3 among keys that sum to 1/8: the target cuts after the third,
    the fourth (the first key of chunk 1) and the fifth tie."""
    cols = 2 * C + 1
    q = P.softmax_of(np.random.default_rng(0x70C5).standard_normal((1, cols))) / 8
    q[0, C - 3:C + 4] = 0.125
    x = np.ascontiguousarray(np.broadcast_to(P.words_of(q, kind), (3, cols)))
    at = np.arange(C - 3, C + 4)
    p = np.array([0.36, 0.45, 0.6], dtype=np.float32)  # of a total of about 1: 3, 4 and 5 ties
    gk, gm, gc = check(ls, torch_gpu, x, p, kind, cross=True)
    for r, c in enumerate((3, 4, 5)):
        assert gc[r] == c and gm[r, at].tolist() == [1] * c + [0] * (7 - c)


@KINDS
def test_every_level_decides_once(ls, torch_gpu, kind):
    """Rows whose keys share the top 8, 16 or 24 bits of the image (the 16-bit types: the top 8): the
    levels above the first differing digit pick the one digit that holds all of the mass."""
    rng = np.random.default_rng(0x70C6)
    for cols in (1000, 2 * C + 1):
        if R.is16(kind):
            base = 0x3C00 if kind == "bf16" else 0x2C00  # 2^-7, 2^-4
            x = (base + rng.integers(0, 256, size=(1, cols))).astype(np.uint16)
        else:
            x = np.stack([(0x3C123400 & (0xFFFFFFFF << b)) + rng.integers(0, 1 << b, size=cols) for b in (24, 16, 8)]).astype(np.uint32)
        u = R.u_of(x, kind, True).astype(np.uint32)
        if R.is16(kind):
            u = u << np.uint32(16)  # (the image the kernels work on)
        for r in range(x.shape[0]):
            assert int((u[r] ^ u[r, 0]).max()) >> (24, 16, 8)[r] == 0 and np.unique(u[r]).size > 100
        for p in (0.5, 0.9, 1.0):
            check(ls, torch_gpu, x, p, kind)


@KINDS
@pytest.mark.parametrize("cols", [300, C + 1])
def test_special_values(ls, torch_gpu, cols, kind):
    wd = R.wdtype(kind)
    sign = 0x8000 if R.is16(kind) else 0x80000000
    base = P.softmax_words(cols, kind, 0x70C7 + cols, rows=1)[0]
    nans = np.array({"f32": [0xFFC00001, 0x7FC00000, 0xFF800001, 0x7FFFFFFF], "bf16": [0xFFC1, 0x7FC0, 0xFF81, 0x7FFF],
                     "f16": [0xFE01, 0x7E00, 0xFC01, 0x7FFF]}[kind]).astype(wd)
    at = np.array([3, cols // 2, cols // 2 + 1, cols - 1])
    # NaNs are kept, weigh nothing and do not move the count: against the row with zeros in their place
    x = np.stack([base, base])
    x[0, at] = nans
    x[1, at] = 0
    for p in (2.0 ** -30, 0.5, 1.0):
        gk, gm, gc = check(ls, torch_gpu, x, p, kind, fill=5)
        assert gc[0] == gc[1] + 4 and gm[0, at].tolist() == [1] * 4 and gm[1, at].tolist() == [0] * 4
        keep = np.ones(cols, dtype=bool)
        keep[at] = False
        np.testing.assert_array_equal(gm[0, keep], gm[1, keep])
    # +inf and values above 1 weigh 1 each, in the order of their keys: +inf, 3, 1.5, 1
    inf = {"f32": 0x7F800000, "bf16": 0x7F80, "f16": 0x7C00}[kind]
    big = np.array([ONE[kind], inf, P.words_of(np.array([3.0]), kind)[0], P.words_of(np.array([1.5]), kind)[0]]).astype(wd)
    x = base.reshape(1, cols).copy()
    x[0, at] = big
    assert P.weight(big, kind).tolist() == [P.ONE] * 4
    for p, k in ((0.1, 1), (0.3, 2), (0.5, 3), (0.7, 4)):  # of a total of 5 and a little less
        gk, gm, gc = check(ls, torch_gpu, x, p, kind)
        assert gc[0] == k and np.flatnonzero(gm[0]).tolist() == sorted(at[[1, 2, 3, 0][:k]].tolist())
    # negatives, -0.0, +0.0, subnormals and values below 2^-40 are never kept, not even at p = 1
    tiny = {"f32": [0x2B7FFFFF, 0x00000001, 0x007FFFFF, 0x00800000], "bf16": [0x2B7F, 0x0001, 0x007F, 0x0080],
            "f16": [0, 0, 0, 0]}[kind]  # (float16's smallest subnormal is 2^-24: it has a weight)
    dead = np.array([sign, 0, sign | ONE[kind], sign | inf] + tiny).astype(wd)
    assert not P.weight(dead, kind).any()
    x = base.reshape(1, cols).copy()
    dat = np.arange(0, 8) * (cols // 8) + 1
    x[0, dat] = dead
    gk, gm, gc = check(ls, torch_gpu, x, 1.0, kind, fill=int(ONE[kind]))
    assert not gm[0, dat].any() and gc[0] <= cols - 8
    if kind == "f16":
        x[0, dat[:2]] = np.array([0x0001, 0x03FF], dtype=wd)  # subnormals with a weight: kept at p = 1
        gk, gm, gc = check(ls, torch_gpu, x, 1.0, kind)
        assert gm[0, dat[:2]].tolist() == [1, 1]


@KINDS
@pytest.mark.parametrize("cols", [1000, 2 * C + 1])
def test_rows_without_mass_and_bad_p(ls, torch_gpu, cols, kind):
    """A row of zeros, negatives and a NaN between two ordinary rows is kept whole and reported; a d_p of
    0, -1, 1.5 and NaN is clamped and reported; the other rows are exact either way."""
    x = P.special_rows(kind, cols, 0x70C8 + cols)[[0, 2, 3]]
    x[1, 7] = R.nan_word(kind)
    want = P.by_threshold(x, 0.9, kind, 9)
    assert want[3] and want[2][1] == cols and want[2][0] < cols and want[2][2] < cols
    gk, gm, gc = check(ls, torch_gpu, x, 0.9, kind, fill=9, want=want)
    assert bool((gm[1] == 1).all())
    check(ls, torch_gpu, x[[0, 2]], 0.9, kind, fill=9)  # (the same rows without it: no report)
    x = P.special_rows(kind, cols, 0x70C9 + cols)[[0, 1, 3, 0, 1, 3]]
    p = np.array([0.5, 0.0, -1.0, 1.5, np.nan, 0.25], dtype=np.float32)
    want = P.by_threshold(x, p, kind, 0)
    assert want[3]
    gk, gm, gc = check(ls, torch_gpu, x, p, kind, want=want)
    one = P.by_threshold(x, np.array([0.5, 2.0 ** -32, 2.0 ** -32, 1.0, 1.0, 0.25], dtype=np.float32), kind, 0)
    assert not one[3]
    np.testing.assert_array_equal(gc, one[2])
    p[4] = -np.nan
    check(ls, torch_gpu, x, p, kind, want=want, keys=False)


@KINDS
def test_output_combinations(ls, torch_gpu, kind):
    """Each output alone, each pair and all three give the same words, mask and counts, and an output
    that is not asked for is not written (run() checks its whole storage), on both paths."""
    for rows, cols in ((3, 4097), (2, 2 * C + 1)):
        x = P.special_rows(kind, cols, 0x70CA + cols)[[0, 1, 3][:rows]]
        for p in (0.9, rows_p(rows, 0x70CB)):
            want = P.by_threshold(x, p, kind, 1)
            for keys, mask, kept in ((True, True, True), (True, False, False), (False, True, False), (False, False, True),
                                     (True, False, True), (False, True, True), (True, True, False)):
                check(ls, torch_gpu, x, p, kind, fill=1, want=want, keys=keys, mask=mask, kept=kept)


@KINDS
def test_in_place(ls, torch_gpu, kind):
    """d_keys_out == d_keys, short and long rows: what the out-of-place call gives."""
    for rows, cols in ((4, 1000), (3, 4097), (3, C), (2, C + 1), (3, 3 * C - 1)):
        x = P.special_rows(kind, cols, 0x70CC + cols)[:rows]  # (from three rows on: one without mass)
        for p in (0.75, rows_p(rows, 0x70CD)):
            want = P.by_threshold(x, p, kind, 0)
            ok, om, oc = check(ls, torch_gpu, x, p, kind, want=want)
            ik, im, ic = check(ls, torch_gpu, x, p, kind, want=want, inplace=True)
            np.testing.assert_array_equal(ik, ok)
            np.testing.assert_array_equal(im, om)
            np.testing.assert_array_equal(ic, oc)
        check(ls, torch_gpu, x, 0.5, kind, inplace=True, mask=False, kept=False)


PHASE_ROWS = 9  # odd rows of odd length: every row starts at another phase, the neighbours run at the same time


@KINDS
@pytest.mark.parametrize("cols", [63, 4097, 2 * C + 1])
def test_phases(ls, torch_gpu, cols, kind):
    """Rows of odd length share their first and last 4 and 16 bytes with their neighbours.  The input at
    every phase inside its 16 bytes; the keys output at the same phase (16-byte stores), at another
    (element stores) and in place; the mask at phases of its own."""
    x = np.concatenate([P.special_rows(kind, cols, 0x70CE + cols + i)[[0, 1, 3]] for i in range(3)])
    assert x.shape[0] == PHASE_ROWS
    p = rows_p(PHASE_ROWS, 0x70CF)
    want = P.by_threshold(x, p, kind, 2)
    E = 8 if R.is16(kind) else 4
    for in_off in range(E):
        check(ls, torch_gpu, x, p, kind, fill=2, want=want, in_off=in_off, mask_off=(3 * in_off + 1) % 8)
        check(ls, torch_gpu, x, p, kind, fill=2, want=want, in_off=in_off, out_off=(in_off + 3) % E, mask=False, kept=False)
        check(ls, torch_gpu, x, p, kind, fill=2, want=want, in_off=in_off, inplace=True, mask=in_off % 2 == 0)


@KINDS
def test_the_same_call_twice(ls, torch_gpu, kind):
    """Integer masses: atomics cannot change a result.  Two calls, identical bytes, on both paths."""
    for rows, cols in ((5, 4097), (3, 3 * C - 1)):
        x = P.softmax_words(cols, kind, 0x70D0 + cols, 0.7, rows=rows)
        x[0, ::7] = x[0, 3]
        p = rows_p(rows, 0x70D1)
        a = run(ls, torch_gpu, x, p, kind)
        b = run(ls, torch_gpu, x, p, kind)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("cols", [4097, 2 * C + 1])
def test_graph_replay(ls, torch_gpu, cols, kind):
    """A call with d_p captured once on a side stream and replayed on new keys and new p values in the
    same buffers.  The launch sequence is linear."""
    torch = torch_gpu
    rows = 3
    sd = sdtype(torch, kind)
    src = torch.zeros((rows, cols), dtype=sd, device="cuda")
    dp = torch.ones((rows,), dtype=torch.float32, device="cuda")
    ko = torch.zeros((rows, cols), dtype=sd, device="cuda")
    mo = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda")
    co = torch.zeros((rows,), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.top_p_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.top_p_device(src, rows, cols, dp, ko, mo, co, fill_bits=4, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.top_p_device(src, rows, cols, dp, ko, mo, co, fill_bits=4, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    rng = np.random.default_rng(0x70D2)
    for i in range(3):
        x = P.special_rows(kind, cols, 0x70D3 + i)[[0, 1, 3]]
        p = np.maximum(rng.random(rows).astype(np.float32), np.float32(2.0 ** -20))
        src.copy_(to_dev(torch, x, kind))
        dp.copy_(torch.from_numpy(p))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.top_p_workspace_status(ws)
        ek, em, ec, flagged = P.by_threshold(x, p, kind, 4)
        assert not flagged
        np.testing.assert_array_equal(co.cpu().numpy().astype(np.int64), ec)
        np.testing.assert_array_equal(mo.cpu().numpy(), em)
        R.assert_keys(ko.cpu().numpy().view(R.wdtype(kind)), ek, kind, f"replay {i}")


SWEEP_SEED = 137
SWEEP_CASES = 36


def sweep_cases(seed):
    """SWEEP_CASES cases: cols log-uniform in [1, 3C], a third of the cases on m C + {-1, 0, 1}; 1 .. 5
    rows; every kind; every row from its own generator of sort_sweep_model, in even cases as the logits
    of a softmax (clipped to +-30, a NaN as 0), in odd ones as the weights themselves (NaNs, negatives
    and values above 1 among them); the outputs, in place and the phases random; half of the cases with
    a random p per row."""
    for i in range(SWEEP_CASES):
        rng = np.random.default_rng([seed, 0x70D4, i])
        if i % 3 == 0:
            cols = min(max(int(rng.integers(1, 4)) * C + int(rng.integers(-1, 2)), 1), 3 * C)
        else:
            cols = min(max(int(np.exp(rng.uniform(0.0, np.log(3 * C)))), 1), 3 * C)
        rows = int(rng.integers(1, 6))
        kind = P.KINDS[int(rng.integers(0, len(P.KINDS)))]
        keys, mask, kept = ((True, True, True), (True, False, True), (False, True, False), (False, False, True))[int(rng.integers(0, 4))]
        inplace = keys and bool(rng.integers(0, 2))
        in_off, mask_off = int(rng.integers(0, 8 if R.is16(kind) else 4)), int(rng.integers(0, 8))
        gens = [S.pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([S.sweep_row(g, cols, kind, True, rng) for g in gens]).astype(R.wdtype(kind))
        if i % 2 == 0:
            with np.errstate(invalid="ignore"):
                z = np.nan_to_num(P.widen(x, kind).view(np.float32).astype(np.float64), nan=0.0, posinf=30.0, neginf=-30.0)
            x = P.words_of(P.softmax_of(np.clip(z, -30.0, 30.0)), kind)
        p = np.maximum(rng.random(rows).astype(np.float32), np.float32(2.0 ** -32)) if i % 4 < 2 else float(np.float32(rng.uniform(0.01, 1.0)))
        tag = f"seed={seed} case={i} {kind} ({rows}, {cols}) p={p} keys={keys} mask={mask} kept={kept} inplace={inplace} in_off={in_off} mask_off={mask_off} rows={gens}"
        yield dict(x=x, p=p, kind=kind, tag=tag,
                   kw=dict(keys=keys, mask=mask, kept=kept, inplace=inplace, in_off=in_off, mask_off=mask_off))


def test_seeded_sweep(ls, torch_gpu):
    """One workspace, filled with 0xFF once and never cleared between the cases."""
    torch = torch_gpu
    cases = list(sweep_cases(SWEEP_SEED))
    assert len(cases) == SWEEP_CASES
    ws = torch.full((max(ls.top_p_workspace_bytes(*c["x"].shape) for c in cases),), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths = [], {"short": 0, "long": 0}
    for c in cases:
        paths["short" if c["x"].shape[1] <= ls.kth_row_keys() else "long"] += 1
        try:
            check(ls, torch, c["x"], c["p"], c["kind"], ws=ws, **c["kw"])
        except AssertionError as err:
            failures.append(f"{c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {SWEEP_SEED}: {paths}")
    assert paths["short"] >= 5 and paths["long"] >= 5
    assert not failures, failures


@KINDS
def test_python_top_p_filter_and_mask(ls, torch_gpu, kind):
    """ls.top_p_filter and ls.top_p_mask against the model: a float p and a tensor p, the default and a
    given fill, out=None, another tensor and x itself, return_kept, a 1-D tensor; and the TypeErrors that
    need a CUDA x."""
    torch = torch_gpu
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]
    for rows, cols in ((4, 1000), (3, 2 * C + 1)):
        xw = P.softmax_words(cols, kind, 0x70D5 + cols, rows=rows)
        x = to_dev(torch, xw, kind).cuda().view(dt)
        pt = torch.tensor([1.0, 0.5, 0.9, 0.1][:rows], dtype=torch.float32, device="cuda")
        for p in (0.9, pt):
            pm = 0.9 if isinstance(p, float) else pt.cpu().numpy()
            for fill in (0.0, -1.0):
                fb = int(P.words_of(np.array([fill]), kind)[0])
                ek, em, ec, _ = P.by_threshold(xw, pm, kind, fb)
                got = ls.top_p_filter(x, p, fill=fill)
                assert got.dtype == x.dtype and got.shape == x.shape and got.data_ptr() != x.data_ptr()
                np.testing.assert_array_equal(got.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), ek)
                out = torch.empty_like(x)
                res, kept = ls.top_p_filter(x, p, fill=fill, out=out, return_kept=True)
                assert res is out and kept.dtype == torch.int32 and kept.cpu().numpy().tolist() == ec.tolist()
                np.testing.assert_array_equal(out.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), ek)
                y = x.clone()
                assert ls.top_p_filter(y, p, fill=fill, out=y) is y
                np.testing.assert_array_equal(y.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), ek)
            m, kept = ls.top_p_mask(x, p, return_kept=True)
            assert m.dtype == torch.bool and m.shape == x.shape and kept.cpu().numpy().tolist() == ec.tolist()
            np.testing.assert_array_equal(m.cpu().numpy().astype(np.uint8), em)
            assert torch.equal(ls.top_p_mask(x, p), m)
        row = x[1].contiguous()  # 1-D: one row
        got = ls.top_p_filter(row, 0.5)
        assert got.shape == row.shape and int(ls.top_p_mask(row, 0.5).sum()) == int(P.by_threshold(xw[1:2], 0.5, kind, 0)[2][0])
        for badp in (pt.to(torch.float64), pt[:2], pt.cpu(), pt.view(1, -1), "0.5", None, True, torch.ones(rows, dtype=torch.int32, device="cuda")):
            for f in (ls.top_p_filter, ls.top_p_mask):
                with pytest.raises(TypeError):
                    f(x, badp)
        for bad_out in (torch.empty_like(x).to(torch.float64), torch.empty((rows, cols + 1), dtype=x.dtype, device="cuda"),
                        torch.empty((cols, rows), dtype=x.dtype, device="cuda").t(), torch.empty(x.shape, dtype=x.dtype), "out"):
            with pytest.raises(TypeError):
                ls.top_p_filter(x, 0.5, out=bad_out)
        for bad in (0.0, 1.5, float("nan")):
            with pytest.raises(ls.LabsortError):
                ls.top_p_filter(x, bad)  # the host p is checked before any launch
        with pytest.raises(ls.LabsortError) as e:
            ls.top_p_mask(x, torch.zeros(rows, dtype=torch.float32, device="cuda"))  # a device p: reported by the status
        assert e.value.status == ls.ERR_ARG
