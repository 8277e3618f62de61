"""labsort_sample_device on the GPU: positions drawn from every row by exact inverse CDF, against the
numpy model of the contract (tests/sample_model.py) bit for bit, for the three key types, at the smallest
shapes at which the two paths -- one workgroup per row up to C = kth_row_keys() keys; chunk masses, a
pick per row and a search per draw above -- can go wrong.  Every call runs on a workspace filled with
0xFF unless it is given one, on positions between guard words that must keep their pattern, is followed
by the status call, and must leave the input and d_u as they were."""
import numpy as np
import pytest

import rowsort_model as R
import sample_model as M
import sort_sweep_model as S
import top_p_model as P
import topk_model as T

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", P.KINDS)
IPAT, GUARD = 0x5A5A5A5A, 8
C = T.constants()["TK_CHUNK"]
ONE = {"f32": 0x3F800000, "bf16": 0x3F80, "f16": 0x3C00}
WORD_CAP = 4096


def to_dev(torch, x, kind):
    sd = np.int16 if R.is16(kind) else np.int32
    return torch.from_numpy(np.array(x).view(sd))  # (a writable copy)


def u_dev(torch, U):
    return torch.from_numpy(np.asarray(U).astype(np.uint32).view(np.int32)).cuda()


def words(seed, rows, ndraw):
    """Seeded random words (uint64 holding [0, 2^32)) with the words 0 and 0xFFFFFFFF among them: in every
    row from three draws on, else spread over the rows."""
    U = np.random.default_rng(seed).integers(0, 1 << 32, size=(rows, ndraw), dtype=np.uint64)
    if ndraw >= 3:
        U[:, 0], U[:, -1] = 0, 0xFFFFFFFF
    else:
        U[0, 0] = 0
        if rows > 1:
            U[1, -1] = 0xFFFFFFFF
    return U


def run(ls, torch, x, U, kind, in_off=0, ws=None, status=0):
    """in_off: elements between an aligned address and the matrix.  Returns the uint32 positions."""
    rows, cols = x.shape
    ndraw = U.shape[1]
    n, nd = rows * cols, rows * ndraw
    sd = torch.int16 if R.is16(kind) else torch.int32
    store = torch.full((GUARD + in_off + n + GUARD,), 0x1111, dtype=sd, device="cuda")
    d = store[GUARD + in_off:GUARD + in_off + n]
    d.copy_(to_dev(torch, x, kind).reshape(-1))
    before = store.clone()
    ud = u_dev(torch, U)
    ubefore = ud.clone()
    ostore = torch.full((GUARD + nd + GUARD,), IPAT, dtype=torch.int32, device="cuda")
    out = ostore[GUARD:GUARD + nd]
    if ws is None:
        ws = torch.full((ls.sample_workspace_bytes(rows, cols, ndraw),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sample_device(d, rows, cols, ud, ndraw, out, key=kind, workspace=ws)
    assert ls.lib.labsort_sample_workspace_status(ws.data_ptr(), None) == status
    assert torch.equal(store, before), "the input was written"
    assert torch.equal(ud, ubefore), "d_u was written"
    assert bool((ostore[:GUARD] == IPAT).all()) and bool((ostore[GUARD + nd:] == IPAT).all()), "written outside the positions"
    assert not bool((out == IPAT).any()), "a position was not written"
    return out.cpu().numpy().view(np.uint32).reshape(rows, ndraw)


def check(ls, torch, x, U, kind, want=None, **kw):
    """want: the model's (positions, flagged) when the test computed it already."""
    exp, flagged = M.draw(x, U, kind) if want is None else want
    got = run(ls, torch, x, U, kind, status=ls.ERR_ARG if flagged else ls.OK, **kw)
    np.testing.assert_array_equal(got, exp, err_msg=f"{kind} {x.shape} ndraw={U.shape[1]} {kw}")
    return got


def test_shapes(ls):
    assert ls.kth_row_keys() == C == 16384


SHORT = [1, 2, 7, 8, 9, 255, 256, 4095, 4096, 4097, C - 1, C]


@KINDS
@pytest.mark.parametrize("cols", SHORT)
def test_short_rows(ls, torch_gpu, cols, kind):
    """4096 / 4097: the last row of the 256-thread workgroup and the first of the 1024-thread one; C: the
    longest row one workgroup holds.  Three rows, so that odd lengths put them at different 16-byte
    phases; a softmax row and two with NaNs, values above 1, negatives, zeros, tiny values and a tie
    block planted (of one or two columns some have no mass: the model says which)."""
    assert ls.sample_workspace_bytes(3, cols, 1000) == 256
    x = P.special_rows(kind, cols, 0x5A40 + cols)[[0, 1, 3]]
    w = P.weight(x, kind)
    for ndraw in (1, 3) + ((1000,) if cols in (4097, C) else ()):
        check(ls, torch_gpu, x, words(0x5A41 + cols + ndraw, 3, ndraw), kind, want=M.draw_weights(w, words(0x5A41 + cols + ndraw, 3, ndraw)))


@KINDS
def test_input_phases(ls, torch_gpu, kind):
    """Rows of odd length with the matrix at every element phase inside its 16 bytes."""
    cols = 255
    x = np.concatenate([P.special_rows(kind, cols, 0x5A42 + i)[[0, 1, 3]] for i in range(3)])
    U = words(0x5A43, 9, 3)
    want = M.draw(x, U, kind)
    for in_off in range(8 if R.is16(kind) else 4):
        check(ls, torch_gpu, x, U, kind, want=want, in_off=in_off)


@KINDS
@pytest.mark.parametrize("which", ["C+1", "2C", "2C+1", "3C-1"])
def test_long_rows(ls, torch_gpu, which, kind):
    """C + 1: the first long row, whose last chunk holds one key."""
    cols = {"C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1}[which]
    assert ls.sample_workspace_bytes(2, cols, 1) > 256
    x = P.special_rows(kind, cols, 0x5A44 + cols)[[0, 3]]
    w = P.weight(x, kind)
    for ndraw in (1, 5):
        U = words(0x5A45 + cols + ndraw, 2, ndraw)
        check(ls, torch_gpu, x, U, kind, want=M.draw_weights(w, U))
    U = np.array([[0xFFFFFFFF], [0]], dtype=np.uint64)  # (the last key of the last chunk; the first of the first)
    check(ls, torch_gpu, x, U, kind, want=M.draw_weights(w, U))


def test_the_longest_row(ls, torch_gpu):
    """One bfloat16 row of 2^23 columns, 512 chunks: its mass spread, only in the last element, and only
    in chunk 300."""
    cols, kind = 1 << 23, "bf16"
    rng = np.random.default_rng(0x5A46)
    spread = P.words_of(rng.random(cols, dtype=np.float32) * np.float32(2.0 ** -18), kind)
    w = P.weight(spread, kind).reshape(1, cols)
    assert ls.sample_workspace_bytes(1, cols, 6) == 256 + 512 * 8 + 256
    U = words(0x5A47, 1, 6)
    got = check(ls, torch_gpu, spread.reshape(1, cols), U, kind, want=M.draw_weights(w, U))
    assert got[0, 0] < C and got[0, -1] >= 511 * C
    last = np.zeros((1, cols), dtype=np.uint16)
    last[0, -1] = spread[7]
    wl = np.zeros((1, cols), dtype=np.uint64)
    wl[0, -1] = w[0, 7]
    assert wl[0, -1] > 0
    got = check(ls, torch_gpu, last, U, kind, want=M.draw_weights(wl, U))
    assert (got == cols - 1).all()
    only = np.zeros((1, cols), dtype=np.uint16)
    only[0, 300 * C:301 * C] = spread[300 * C:301 * C]
    wo = np.zeros((1, cols), dtype=np.uint64)
    wo[0, 300 * C:301 * C] = w[0, 300 * C:301 * C]
    got = check(ls, torch_gpu, only, U, kind, want=M.draw_weights(wo, U))
    assert (got // C == 300).all()


def test_more_workgroups_than_one_grid_holds(ls, torch_gpu):
    """The contract allows rows and rows x ndraw up to 2^31 - 1, one workgroup each, and the runtime
    takes no grid of 2^32 threads: the smallest calls past that on each path.  Short rows: 2^24 + 3 rows of
    one column (256 threads a row), every fifth without mass.  Long rows: two all-equal rows of C + 1
    columns at 2^21 + 1 draws each (1024 threads a draw), where word U draws floor(U cols / 2^32)."""
    rng = np.random.default_rng(0x5A5F)
    rows = (1 << 24) + 3
    assert rows * 256 >= 1 << 32
    x = np.full((rows, 1), P.words_of(np.array([0.5]), "f32")[0], dtype=np.uint32)
    x[::5] = 0
    assert P.weight(x[:2, 0], "f32").tolist() == [0, P.ONE >> 1]
    U = rng.integers(0, 1 << 32, size=(rows, 1), dtype=np.uint64)
    got = run(ls, torch_gpu, x, U, "f32", status=ls.ERR_ARG)
    np.testing.assert_array_equal(got, np.where(x != 0, 0, M.SENTINEL).astype(np.uint32))
    rows, cols, ndraw = 2, C + 1, (1 << 21) + 1
    assert rows * ndraw * 1024 >= 1 << 32
    x = np.full((rows, cols), P.words_of(np.array([1.0 / 1024]), "f32")[0], dtype=np.uint32)
    U = rng.integers(0, 1 << 32, size=(rows, ndraw), dtype=np.uint64)
    U[:, 0], U[:, -1] = 0, 0xFFFFFFFF
    got = run(ls, torch_gpu, x, U, "f32")
    np.testing.assert_array_equal(got, ((U * np.uint64(cols)) >> np.uint64(32)).astype(np.uint32))
    assert got[0, -1] == cols - 1 and got[1, 0] == 0


def boundary_words(x_row, kind, seed, must=()):
    """WORD_CAP words of one row: U_b - 1 and U_b of its boundaries (sample_model.boundaries; a U_b of 2^32
    is no word), all of them if they fit, else the first two, the last two, those of the cumulative
    masses `must` and a seeded sample; padded with random words.  Returns (words, how many were left out)."""
    ub, cs = M.boundaries(x_row, kind)
    every = sorted({u for b in ub for u in (b - 1, b) if u < (1 << 32)})
    keep = {u for b, c in zip(ub, cs) if c in must for u in (b - 1, b) if u < (1 << 32)}
    keep |= set(every[:2] + every[-2:])
    assert len(keep) <= WORD_CAP
    rng = np.random.default_rng(seed)
    rest = [u for u in every if u not in keep]
    if len(keep) + len(rest) > WORD_CAP:
        rest = [rest[i] for i in rng.choice(len(rest), size=WORD_CAP - len(keep), replace=False)]
    chosen = sorted(keep) + rest
    pad = rng.integers(0, 1 << 32, size=WORD_CAP - len(chosen), dtype=np.uint64).tolist()
    return np.array(chosen + pad, dtype=np.uint64), len(every) - len(chosen)


@KINDS
@pytest.mark.parametrize("cols", [9, 4097])
def test_every_boundary_of_a_short_row(ls, torch_gpu, cols, kind):
    """U_b - 1 and U_b for all cumulative masses of a 9-column row (16 words, none left out) and of a
    4097-column row, which has 2 x 4096 such words: 4096 are run (the first, the last and a seeded sample)
    and 4096 left out; the count is asserted below."""
    x = P.softmax_words(cols, kind, 0x5A48 + cols, rows=1)
    U, left = boundary_words(x[0], kind, 0x5A49)
    print(f"{kind} cols={cols}: {left} boundary words left out")
    assert left == {9: 0, 4097: 4096}[cols]
    check(ls, torch_gpu, x, U.reshape(1, -1), kind)


@KINDS
def test_chunk_edge_boundaries(ls, torch_gpu, kind):
    """A 2C + 1 row: the boundaries at the two chunk edges (the draw moves from the last key of a chunk to
    the first of the next), and, in a second row whose chunk 1 has no mass at all, the one boundary
    between the last key of chunk 0 and the first of chunk 2.  All chunk-edge boundaries are in; of the
    2 x 2C other boundary words per row a seeded sample fills the 4096 (about 61000 are left out per row)."""
    cols = 2 * C + 1
    x = P.softmax_words(cols, kind, 0x5A4A, rows=2)
    x[1, C:2 * C] = 0
    w = P.weight(x, kind)
    assert w[0].all() and w[1, :C].all() and w[1, 2 * C:].all()
    cum = np.cumsum(w, axis=1, dtype=np.uint64)
    must = [(int(cum[0, C - 1]), int(cum[0, 2 * C - 1])), (int(cum[1, C - 1]),)]
    assert int(cum[1, C - 1]) == int(cum[1, 2 * C - 1])
    rows = []
    for r in range(2):
        U, left = boundary_words(x[r], kind, 0x5A4B + r, must=must[r])
        print(f"{kind} row {r}: {left} boundary words left out")
        ub, cs = M.boundaries(x[r], kind)
        for c in must[r]:
            b = ub[cs.index(c)]
            assert b - 1 in U and b in U
        rows.append(U)
    U = np.stack(rows)
    got = check(ls, torch_gpu, x, U, kind, want=M.draw_weights(w, U))
    # the edges themselves: the last key of a chunk at U_b - 1, the first key with mass behind it at U_b
    for r, c, (a, b) in ((0, must[0][0], (C - 1, C)), (0, must[0][1], (2 * C - 1, 2 * C)), (1, must[1][0], (C - 1, 2 * C))):
        ub, cs = M.boundaries(x[r], kind)
        e = ub[cs.index(c)]
        assert got[r][U[r] == e - 1].tolist() == [a] and got[r][U[r] == e].tolist() == [b]


@KINDS
@pytest.mark.parametrize("cols", [300, C + 1])
def test_special_values(ls, torch_gpu, cols, kind):
    """NaNs, +inf and values above 1 (weight 2^40), negatives, both zeros, subnormals and values below
    2^-40, and leading and trailing runs of zero weight: what has no weight is never drawn."""
    wd = R.wdtype(kind)
    sign = 0x8000 if R.is16(kind) else 0x80000000
    inf = {"f32": 0x7F800000, "bf16": 0x7F80, "f16": 0x7C00}[kind]
    nans = {"f32": [0xFFC00001, 0x7FC00000, 0xFF800001, 0x7FFFFFFF], "bf16": [0xFFC1, 0x7FC0, 0xFF81, 0x7FFF],
            "f16": [0xFE01, 0x7E00, 0xFC01, 0x7FFF]}[kind]
    tiny = {"f32": [0x2B7FFFFF, 0x00000001, 0x007FFFFF, 0x00800000], "bf16": [0x2B7F, 0x0001, 0x007F, 0x0080],
            "f16": [0x0001, 0x03FF, 0, 0]}[kind]  # (float16's subnormals have weights: 2^-24 and up)
    big = [ONE[kind], inf, int(P.words_of(np.array([3.0]), kind)[0]), ONE[kind] + 5]
    dead = [sign, 0, sign | ONE[kind], sign | inf]
    plant = np.array(nans + tiny + big + dead).astype(wd)
    x = P.softmax_words(cols, kind, 0x5A4C + cols, rows=3)
    at = np.random.default_rng(0x5A4D).choice(np.arange(8, cols - 8), size=plant.size, replace=False)
    x[0, at] = plant
    x[1, at] = plant[::-1]
    x[:2, :7], x[:2, -6:] = 0, sign  # leading and trailing runs without weight
    w = P.weight(x, kind)
    assert P.weight(np.array(big).astype(wd), kind).tolist() == [P.ONE] * 4
    assert not P.weight(np.array(nans + dead).astype(wd), kind).any()
    U = np.concatenate([words(0x5A4E + cols, 3, 200), np.stack([boundary_words(x[r], kind, 0x5A4F)[0][:300] for r in range(3)])], axis=1)
    got = check(ls, torch_gpu, x, U, kind, want=M.draw_weights(w, U))
    for r in range(3):
        assert w[r][got[r].astype(np.int64)].all()
    assert got[0, 0] == 7 and got[0, 199] == cols - 7
    assert np.isin(at[8:12], got[0]).all()  # (each of the four weighs 2^40 of a total of about 4 x 2^40)


@KINDS
@pytest.mark.parametrize("cols", [4097, 2 * C + 1])
def test_one_element_holds_the_mass(ls, torch_gpu, cols, kind):
    """At position 0, at the middle and at cols - 1: every word draws it."""
    x = np.zeros((3, cols), dtype=R.wdtype(kind))
    at = [0, cols // 2, cols - 1]
    for r in range(3):
        x[r, at[r]] = P.words_of(np.array([0.001 * (r + 1)]), kind)[0]
    got = check(ls, torch_gpu, x, words(0x5A50, 3, 9), kind)
    assert (got == np.array(at, dtype=np.uint32).reshape(3, 1)).all()


@KINDS
@pytest.mark.parametrize("cols", [1000, 2 * C + 1])
def test_all_equal_rows(ls, torch_gpu, cols, kind):
    """Every element weighs 2^30: word U draws position floor(U cols / 2^32)."""
    word = P.words_of(np.array([1.0 / 1024]), kind)[0]
    x = np.full((2, cols), word, dtype=R.wdtype(kind))
    U = words(0x5A51 + cols, 2, 64)
    got = check(ls, torch_gpu, x, U, kind)
    np.testing.assert_array_equal(got, ((U * np.uint64(cols)) >> np.uint64(32)).astype(np.uint32))


@KINDS
@pytest.mark.parametrize("cols", [1000, 2 * C + 1])
def test_a_row_without_mass(ls, torch_gpu, cols, kind):
    """A row of zeros, negatives and a NaN between two ordinary rows draws the sentinel and is reported;
    the neighbours are exact; the same rows without it report nothing."""
    x = P.special_rows(kind, cols, 0x5A52 + cols)[[0, 2, 3]]
    x[1, 7] = R.nan_word(kind)
    for ndraw in (1, 4):
        U = words(0x5A53 + ndraw, 3, ndraw)
        want = M.draw(x, U, kind)
        assert want[1] and (want[0][1] == M.SENTINEL).all() and (want[0][[0, 2]] < cols).all()
        check(ls, torch_gpu, x, U, kind, want=want)
        check(ls, torch_gpu, x[[0, 2]], U[[0, 2]], kind, want=(want[0][[0, 2]], False))


@KINDS
def test_the_same_call_twice(ls, torch_gpu, kind):
    for rows, cols, ndraw in ((5, 4097, 7), (3, 3 * C - 1, 7)):
        x = P.softmax_words(cols, kind, 0x5A54 + cols, 0.7, rows=rows)
        U = words(0x5A55, rows, ndraw)
        assert run(ls, torch_gpu, x, U, kind).tobytes() == run(ls, torch_gpu, x, U, kind).tobytes()


@KINDS
@pytest.mark.parametrize("cols", [4097, 2 * C + 1])
def test_graph_replay(ls, torch_gpu, cols, kind):
    """A call captured once on a side stream and replayed on new keys and new words in the same
    buffers.  The launch sequence is linear."""
    torch = torch_gpu
    rows, ndraw = 3, 5
    sd = torch.int16 if R.is16(kind) else torch.int32
    src = torch.zeros((rows, cols), dtype=sd, device="cuda")
    ud = torch.zeros((rows, ndraw), dtype=torch.int32, device="cuda")
    out = torch.zeros((rows, ndraw), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sample_workspace_bytes(rows, cols, ndraw),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture (rows without mass: the header word is set)
        ls.sample_device(src, rows, cols, ud, ndraw, out, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.sample_device(src, rows, cols, ud, ndraw, out, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    for i in range(3):
        x = P.special_rows(kind, cols, 0x5A56 + i)[[0, 1, 3]]
        U = words(0x5A57 + i, rows, ndraw)
        src.copy_(to_dev(torch, x, kind))
        ud.copy_(u_dev(torch, U))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.sample_workspace_status(ws)
        exp, flagged = M.draw(x, U, kind)
        assert not flagged
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), exp, err_msg=f"replay {i}")


@KINDS
@pytest.mark.parametrize("cols", [4096, 2 * C + 1])
def test_top_p_then_sample(ls, torch_gpu, cols, kind):
    """The sampler's tail: top_p_filter(x, p, fill=0) in place, then sample_device on the filtered rows.
    Every position drawn lies in top_p_mask(x, p) and is the model's draw on the model's filtered row."""
    torch = torch_gpu
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]
    rows, ndraw = 3, 16
    xw = P.softmax_words(cols, kind, 0x5A58 + cols, rows=rows)
    U = words(0x5A59 + cols, rows, ndraw)
    for p in (0.5, 0.9):
        x = to_dev(torch, xw, kind).cuda().view(dt)
        mask = ls.top_p_mask(x, p).cpu().numpy()
        assert ls.top_p_filter(x, p, fill=0.0, out=x) is x
        filtered = x.view(torch.int16 if R.is16(kind) else torch.int32).cpu().numpy().view(R.wdtype(kind))
        fw, fm, _, flagged = P.by_threshold(xw, p, kind, 0)
        assert not flagged
        np.testing.assert_array_equal(mask.astype(np.uint8), fm)
        np.testing.assert_array_equal(filtered, fw)
        got = check(ls, torch, filtered, U, kind, want=M.draw(fw, U, kind))  # (the device's filtered rows, the model's draw)
        for r in range(rows):
            assert mask[r][got[r].astype(np.int64)].all()


SWEEP_SEED = 151
SWEEP_CASES = 24


def sweep_cases(seed):
    """SWEEP_CASES cases: cols log-uniform in [1, 3C], a third of the cases on m C + {-1, 0, 1}; 1 .. 4
    rows; every kind; every row from its own generator of sort_sweep_model, taken as raw weights (NaNs,
    negatives and values above 1 among them; a row may have no mass); 1 .. 6 draws; the phase random."""
    for i in range(SWEEP_CASES):
        rng = np.random.default_rng([seed, 0x5A5A, i])
        if i % 3 == 0:
            cols = min(max(int(rng.integers(1, 4)) * C + int(rng.integers(-1, 2)), 1), 3 * C)
        else:
            cols = min(max(int(np.exp(rng.uniform(0.0, np.log(3 * C)))), 1), 3 * C)
        rows, ndraw = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        kind = P.KINDS[int(rng.integers(0, len(P.KINDS)))]
        in_off = int(rng.integers(0, 8 if R.is16(kind) else 4))
        gens = [S.pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([S.sweep_row(g, cols, kind, True, rng) for g in gens]).astype(R.wdtype(kind))
        U = rng.integers(0, 1 << 32, size=(rows, ndraw), dtype=np.uint64)
        yield dict(x=x, U=U, kind=kind, in_off=in_off, tag=f"seed={seed} case={i} {kind} ({rows}, {cols}) ndraw={ndraw} in_off={in_off} rows={gens}")


def test_seeded_sweep(ls, torch_gpu):
    """One workspace, filled with 0xFF once and never cleared between the cases."""
    torch = torch_gpu
    cases = list(sweep_cases(SWEEP_SEED))
    assert len(cases) == SWEEP_CASES
    ws = torch.full((max(ls.sample_workspace_bytes(*c["x"].shape, c["U"].shape[1]) for c in cases),), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths = [], {"short": 0, "long": 0}
    for c in cases:
        paths["short" if c["x"].shape[1] <= ls.kth_row_keys() else "long"] += 1
        try:
            check(ls, torch, c["x"], c["U"], c["kind"], in_off=c["in_off"], ws=ws)
        except AssertionError as err:
            failures.append(f"{c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {SWEEP_SEED}: {paths}")
    assert paths["short"] >= 4 and paths["long"] >= 4
    assert not failures, failures


@KINDS
def test_python_sample(ls, torch_gpu, kind):
    """ls.sample with u as int32 words, as float32 in [0, 1) and as None with a seeded generator, a 1-D
    tensor, and the TypeErrors that need a CUDA x."""
    torch = torch_gpu
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]
    for rows, cols in ((4, 1000), (3, 2 * C + 1)):
        ndraw = 6
        xw = P.special_rows(kind, cols, 0x5A5B + cols)[[0, 1, 3, 0][:rows]]
        w = P.weight(xw, kind)
        x = to_dev(torch, xw, kind).cuda().view(dt)
        U = words(0x5A5C + cols, rows, ndraw)
        exp = M.draw_weights(w, U)[0]
        got = ls.sample(x, ndraw, u=u_dev(torch, U))
        assert got.dtype == torch.int32 and tuple(got.shape) == (rows, ndraw)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), exp)
        if hasattr(torch, "uint32"):
            np.testing.assert_array_equal(ls.sample(x, ndraw, u=u_dev(torch, U).view(torch.uint32)).cpu().numpy().view(np.uint32), exp)
        uf = np.random.default_rng(0x5A5D).random((rows, ndraw), dtype=np.float32)
        uf[0, 0], uf[0, 1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        Uf = np.floor(uf.astype(np.float64) * 4294967296.0).astype(np.uint64)
        assert Uf[0, 1] == 0xFFFFFF00
        np.testing.assert_array_equal(ls.sample(x, ndraw, u=torch.from_numpy(uf).cuda()).cpu().numpy().view(np.uint32),
                                      M.draw_weights(w, Uf)[0])
        uf[0, :4] = [-0.5, 1.0, 2.5, np.nan]  # clamped: words 0, 2^32 - 1, 2^32 - 1, and 0 for the NaN
        Uf[0, :4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
        np.testing.assert_array_equal(ls.sample(x, ndraw, u=torch.from_numpy(uf).cuda()).cpu().numpy().view(np.uint32),
                                      M.draw_weights(w, Uf)[0])
        gens = [torch.Generator(device="cuda").manual_seed(0x5A5E) for _ in range(2)]
        a, b = (ls.sample(x, 64, generator=g) for g in gens)
        assert a.dtype == torch.int32 and tuple(a.shape) == (rows, 64) and torch.equal(a, b)
        an = a.cpu().numpy().astype(np.int64)
        for r in range(rows):
            assert w[r][an[r]].all()
        assert tuple(ls.sample(x).shape) == (rows, 1) and tuple(ls.sample(x, 0).shape) == (rows, 0)
        row = x[1].contiguous()  # 1-D: one row
        np.testing.assert_array_equal(ls.sample(row, ndraw, u=u_dev(torch, U[1:2])).cpu().numpy().view(np.uint32), exp[1:2])
        good = u_dev(torch, U)
        for bad_u in (good.cpu(), good[:, :3], good.t().contiguous().t(), good.to(torch.int64), good.to(torch.float64),
                      good.reshape(-1), U, "u"):
            with pytest.raises(TypeError):
                ls.sample(x, ndraw, u=bad_u)
        for bad_n in (-1, 1.5, "3", None, True):
            with pytest.raises(TypeError):
                ls.sample(x, bad_n)
    none = torch.zeros((2, 100), dtype=dt, device="cuda")
    with pytest.raises(ls.LabsortError) as e:
        ls.sample(none, 3)  # rows without mass: reported by the status
    assert e.value.status == ls.ERR_ARG
