"""labsort_kth_device on the GPU: the k-th key of every row and its position against the numpy model of
the contract (tests/kth_model.py: column k - 1 of the rows sorted stably on u(key), or the same by
np.partition and the tie rank), for all five key types, at the smallest shapes at which the two paths
-- one workgroup per row up to R = kth_row_keys() keys, a radix select over chunks of C keys with
chunk skipping above -- can go wrong.  Keys compare bit-exact except that a NaN only has to be a NaN,
positions exactly.  Every call runs on a workspace filled with 0xFF and on outputs between guard
elements filled with a pattern, is followed by the status call, and must leave its input as it was."""
import numpy as np
import pytest

import f16_model as M
import kth_model as K
import rowsort_model as R
import sort_sweep_model as S
import topk_model as T

pytestmark = pytest.mark.gpu

BOTH = [False, True]
KINDS = pytest.mark.parametrize("kind", R.KINDS)
FLOATS = ("f32", "bf16", "f16")
KPAT, IPAT = 0x5A5A, -7
C = T.constants()["TK_CHUNK"]


def sdtype(torch, kind):
    """The storage the words travel in: the library takes addresses."""
    return torch.int16 if R.is16(kind) else torch.int32


def to_dev(torch, x, kind):
    sd = np.int16 if R.is16(kind) else np.int32
    return torch.from_numpy(np.array(x).view(sd))  # (a writable copy: a shared case is read-only)


def run(ls, torch, x, k, largest, kind, ws=None, with_idx=True, in_off=0, status=0):
    """k: an int, or one value per row, which travels as d_k (int32 words on the device).  in_off:
    elements between the start of the storage and the matrix.  The outputs sit between guard elements
    that must keep their pattern.  Returns the keys and the positions (None without)."""
    rows, cols = x.shape
    n = rows * cols
    sd = sdtype(torch, kind)
    store = torch.full((n + in_off + 1,), 0x1111, dtype=sd, device="cuda")
    d = store[in_off:in_off + n]
    d.copy_(to_dev(torch, x, kind).reshape(-1))
    before = store.clone()
    ostore = torch.full((2 + rows + 1,), KPAT, dtype=sd, device="cuda")
    ko = ostore[2:2 + rows]
    istore = torch.full((rows + 2,), IPAT, dtype=torch.int32, device="cuda")
    io = istore[1:1 + rows] if with_idx else None
    if ws is None:
        ws = torch.full((ls.kth_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    if isinstance(k, (int, np.integer)):
        karg, kbefore = int(k), None
    else:
        karg = torch.from_numpy((np.asarray(k, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
        assert karg.shape == (rows,)
        kbefore = karg.clone()
    ls.kth_device(d, rows, cols, karg, ko, io, largest=largest, key=kind, workspace=ws)
    assert ls.lib.labsort_kth_workspace_status(ws.data_ptr(), None) == status
    assert torch.equal(store, before), "the input was written"
    assert kbefore is None or torch.equal(karg, kbefore), "d_k was written"
    assert bool((ostore[:2] == KPAT).all()) and int(ostore[-1]) == KPAT, "written outside the key output"
    assert int(istore[0]) == IPAT and int(istore[-1]) == IPAT, "written outside the position output"
    if not with_idx:
        assert bool((istore == IPAT).all()), "a position was written without d_idx_out"
    gk = ko.cpu().numpy().view(R.wdtype(kind))
    return gk, (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, k, largest, kind, exp=None, with_idx=True, **kw):
    """exp: (keys, positions) of the rows sorted (rowsort_model.expected), when a test has them
    already; else the O(cols) form of the model."""
    rows = x.shape[0]
    if exp is not None:
        ks = K.ks_of(k, rows)
        ek, ei = exp[0][np.arange(rows), ks - 1], exp[1][np.arange(rows), ks - 1]
    else:
        ek, ei = K.by_partition(x, k, largest, kind)
    gk, gi = run(ls, torch, x, k, largest, kind, with_idx=with_idx, **kw)
    K.assert_result(gk, gi, ek, ei, kind, f"{kind} {x.shape} k={k} largest={largest} idx={with_idx}")
    return gk, gi


def test_shapes(ls):
    assert ls.kth_row_keys() == C == 16384


@KINDS
@pytest.mark.parametrize("edge", [0, 1])
def test_path_edge(ls, torch_gpu, edge, kind):
    """cols = R: the longest row one workgroup holds, on the 256-byte workspace; R + 1: the first long
    row, whose last chunk holds one key."""
    cols = ls.kth_row_keys() + edge
    assert (ls.kth_workspace_bytes(3, cols) == 256) == (edge == 0)
    x, exp = R.case(kind, 3, cols)
    for largest in BOTH:
        for k in (1, 2, cols // 2, cols - 1, cols):
            for with_idx in (True, False):
                check(ls, torch_gpu, x, k, largest, kind, exp=exp[largest], with_idx=with_idx)


@KINDS
@pytest.mark.parametrize("cols", [1, 2, 63, 64, 65, 1000, 4096, 4097])
def test_short_rows(ls, torch_gpu, cols, kind):
    """4096 / 4097: the last row of the 256-thread workgroup and the first of the 1024-thread one."""
    x, exp = R.case(kind, 5, cols)
    for largest in BOTH:
        for k in (1, cols):
            check(ls, torch_gpu, x, k, largest, kind, exp=exp[largest])


@KINDS
@pytest.mark.parametrize("which", ["2C", "2C+1", "3C-1"])
def test_chunk_edges(ls, torch_gpu, which, kind):
    cols = {"2C": 2 * C, "2C+1": 2 * C + 1, "3C-1": 3 * C - 1}[which]
    x, exp = R.case(kind, 3, cols)
    for largest in BOTH:
        for k in (1, C, cols // 2 + 1, cols):
            check(ls, torch_gpu, x, k, largest, kind, exp=exp[largest])


TIE_KS = (1, C, C + 1, 2 * C, 3 * C + 5)


@KINDS
def test_ties_across_chunks(ls, torch_gpu, kind):
    """A row of 3C + 5 equal keys: the k-th is at position k - 1, host k and a k per row."""
    cols = 3 * C + 5
    word = R.random_words((1,), 0x4B10, kind)[0]
    x = np.full((1, cols), word, dtype=R.wdtype(kind))
    for largest in BOTH:
        for k in TIE_KS:
            gk, gi = run(ls, torch_gpu, x, k, largest, kind)
            K.assert_result(gk, gi, x[:, 0], np.array([k - 1], dtype=np.uint32), kind, f"k={k} largest={largest}")
        x5 = np.broadcast_to(x, (len(TIE_KS), cols))
        gk, gi = run(ls, torch_gpu, x5, np.array(TIE_KS), largest, kind)
        np.testing.assert_array_equal(gi, np.array(TIE_KS) - 1)


@pytest.mark.parametrize("kind", FLOATS)
def test_all_nan_row(ls, torch_gpu, kind):
    """NaNs of several payloads and both signs are one value: the k-th is at position k - 1 and comes
    back as the canonical NaN."""
    cols = 3 * C + 5
    x = S.sweep_row("all_nan", cols, kind, False, np.random.default_rng(0x4B11)).reshape(1, cols).astype(R.wdtype(kind))
    for largest in BOTH:
        for k in TIE_KS:
            gk, gi = run(ls, torch_gpu, x, k, largest, kind)
            assert int(gi[0]) == k - 1
            assert int(gk[0]) == (0x7FFF if R.is16(kind) else 0x7FFFFFFF)


@KINDS
def test_tie_words_rows(ls, torch_gpu, kind):
    """Heavy ties (eight values, both zeros, NaNs): every k cuts a long run of equal keys that spans
    the chunks."""
    x, exp = R.case(kind, 3, 2 * C + 1, "ties")
    cols = x.shape[1]
    rng = np.random.default_rng(0x4B12)
    for largest in BOTH:
        for k in (1, cols // 7, cols // 2, cols - 1, rng.integers(1, cols + 1, size=3)):
            check(ls, torch_gpu, x, k, largest, kind, exp=exp[largest])


def stale_row(kind, largest, rng):
    """Three chunks of order images.  With N the call's last level (1 for the 16-bit kinds, 3 for the
    others), b the digits 0 .. N - 1 of the k-th key and L its last digit: chunk 0 holds C keys with
    digits 0 .. N - 2 of b and digit N - 1 equal to L (not b[N - 1]), so at level N - 1 its count at
    digit L is C and it holds no key of the bucket chosen there: the last level skips it.  Chunks 1 and
    2 hold the bucket: last digits 0x10, L and 0x70 at random.  A kernel that leaves chunk 0's counts
    of level N - 1 in place sees C phantom ties in front of the k-th key.  Returns the words, and the
    ranks (k) of the first, of one in chunk 1, of one in chunk 2 and of the last key whose last digit is L."""
    bits = T.bits_of(kind)
    dt = np.uint64
    L, b_last = 0x50, 0x40
    lead = 0x2A31 if bits == 32 else 0  # digits 0 .. N - 2 (none for 16 bits)
    head = (dt(lead) << dt(8)) if bits == 32 else dt(0)
    c0 = ((head | dt(L)) << dt(8)) | rng.integers(0, 256, size=C, dtype=dt)
    last = np.array([0x10, L, 0x70], dtype=dt)[rng.integers(0, 3, size=2 * C)]
    c12 = ((head | dt(b_last)) << dt(8)) | last
    u = np.concatenate([c0, c12]).astype(T.word_dtype(kind))
    n10 = int(np.count_nonzero(last == 0x10))
    nL1 = int(np.count_nonzero(last[:C] == L))
    nL = int(np.count_nonzero(last == L))
    assert nL1 > 2 and nL - nL1 > 2
    return T.raw_of(u, kind, largest), [n10 + 1, n10 + nL1 - 1, n10 + nL1 + 2, n10 + nL]


@KINDS
def test_stale_counts(ls, torch_gpu, kind):
    for largest in BOTH:
        row, ks = stale_row(kind, largest, np.random.default_rng(0x4B13))
        u = T.u_of(row, kind, largest)
        assert bool((T.raw_of(u, kind, largest) == row).all())
        x = np.ascontiguousarray(np.broadcast_to(row, (len(ks), row.size)))
        ek, ei = K.by_partition(x, np.array(ks), largest, kind)
        assert bool((ei >= C).all()) and int(ei[1]) < 2 * C <= int(ei[2])  # the k-th keys lie in chunks 1 and 2
        for with_idx in (True, False):
            check(ls, torch_gpu, x, np.array(ks), largest, kind, with_idx=with_idx)
        check(ls, torch_gpu, x[:1], ks[2], largest, kind)


@KINDS
@pytest.mark.parametrize("gen", ["sorted", "reversed"])
def test_skipping_sorted_rows(ls, torch_gpu, gen, kind):
    """5C + 7 keys in order: most chunks die at level 1.  The k-th in the first chunk, at both sides of
    a chunk boundary, and in the last (partial) chunk."""
    cols = 5 * C + 7
    for largest in BOTH:
        row = S.sweep_row(gen, cols, kind, largest, np.random.default_rng(0x4B14)).astype(R.wdtype(kind))
        ks = np.array([1, 5, C, C + 1, 3 * C, 3 * C + 1, 5 * C + 1, cols])
        if gen == "reversed":
            ks = cols + 1 - ks
        x = np.ascontiguousarray(np.broadcast_to(row, (ks.size, cols)))
        gk, gi = check(ls, torch_gpu, x, ks, largest, kind)
        check(ls, torch_gpu, x[:1], int(ks[2]), largest, kind)


@KINDS
def test_skipping_shared_prefix_rows(ls, torch_gpu, kind):
    """Rows of topk_model.row_narrowing_at for every level and for NEVER: keys that share their top
    bytes, so nothing is skipped until late."""
    cols = 2 * C + 1
    bits = T.bits_of(kind)
    levels = list(range(bits // 8 - 1)) + [T.NEVER]
    for largest in BOTH:
        u = np.stack([T.row_narrowing_at(lv, cols, 0x4B15, bits) for lv in levels])
        x = np.ascontiguousarray(T.raw_of(u, kind, largest))
        for k in (1, cols // 2, cols):
            check(ls, torch_gpu, x, k, largest, kind)
        check(ls, torch_gpu, x, np.random.default_rng(0x4B16).integers(1, cols + 1, size=len(levels)), largest, kind)


@KINDS
def test_per_row_k(ls, torch_gpu, kind):
    """7 rows of 2C + 1 with seven different k; then one row's k set to 0 and another's to cols + 1:
    the status call reports ERR_ARG, the other rows are right (the two rows get the clamped k's key),
    the guards are intact."""
    x, exp = R.case(kind, 7, 2 * C + 1)
    cols = x.shape[1]
    ks = np.array([1, cols, 2, cols // 2, C, C + 1, cols - 1])
    for largest in BOTH:
        check(ls, torch_gpu, x, ks, largest, kind, exp=exp[largest])
        bad = ks.copy()
        bad[2], bad[5] = 0, cols + 1
        clamped, which = K.clamp(bad, cols)
        assert which.tolist() == [False, False, True, False, False, True, False]
        gk, gi = run(ls, torch_gpu, x, bad, largest, kind, status=ls.ERR_ARG)
        ek, ei = K.by_sort(x, clamped, largest, kind)
        K.assert_result(gk, gi, ek, ei, kind, "clamped k")
    # the same on the one-launch path, a negative k among them
    x, exp = R.case(kind, 5, 1000)
    bad = np.array([1, -1, 500, 0, 1000])
    gk, gi = run(ls, torch_gpu, x, bad, False, kind, status=ls.ERR_ARG)
    ek, ei = K.by_sort(x, K.clamp(bad, 1000)[0], False, kind)
    K.assert_result(gk, gi, ek, ei, kind, "clamped k, short rows")
    check(ls, torch_gpu, x, np.array([1, 7, 500, 999, 1000]), True, kind, exp=exp[True])


@pytest.mark.parametrize("kind", M.KINDS)
def test_16bit_phases(ls, torch_gpu, kind):
    """(2, 70001) one element into its storage: the rows start on both 2-byte phases of a 4-byte word."""
    x, exp = R.case(kind, 2, 70001)
    for in_off in (0, 1):
        for largest in BOTH:
            check(ls, torch_gpu, x, np.array([35000, 70001]), largest, kind, exp=exp[largest], in_off=in_off)
    x, exp = R.case(kind, 3, 4097)  # the one-launch path: rows 1 and 2 start inside a 16-byte group
    for in_off in (0, 1):
        check(ls, torch_gpu, x, np.array([1, 2048, 4097]), True, kind, exp=exp[True], in_off=in_off)


@pytest.mark.parametrize("kind", ["i32", "bf16"])
def test_one_long_row(ls, torch_gpu, kind):
    """One row of 1024 C + C + 5 keys: the histogram workgroups count two chunks each (1025 chunks
    past TK_MAX_HIST_WG = 1024 workgroups), and the last pick's scan along the chunks takes a full step
    of the block size and a partial one."""
    assert T.constants()["TK_MAX_HIST_WG"] == 1024 and T.constants()["TK_BLOCK"] == 1024
    cols = 1024 * C + C + 5
    x = R.random_words((1, cols), 0x4B17, kind)
    x[0, ::4099] = x[0, 7]
    x[0, -3:] = x[0, 7]  # ties of one key in the first and in the last chunk
    below = int(np.count_nonzero(R.u_of(x, kind)[0] < R.u_of(x[:, 7:8], kind)[0, 0]))
    ties = int(np.count_nonzero(x[0] == x[0, 7]))
    for k, largest in ((1, False), (below + ties, False), (cols // 2, True), (cols, False)):
        check(ls, torch_gpu, x, k, largest, kind)


@KINDS
def test_bit_identity_with_the_row_sort(ls, torch_gpu, kind):
    """(4, 3C - 1): key and position are column k - 1 of ls.sort_rows_device's outputs, bit for bit,
    NaN words included."""
    torch = torch_gpu
    rows, cols = 4, 3 * C - 1
    x, _ = R.case(kind, rows, cols)
    d = to_dev(torch, x, kind).cuda()
    for largest in BOTH:
        ko = torch.empty_like(d)
        io = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
        ls.sort_rows_device(d, rows, cols, ko, io, descending=largest, key=kind)
        sk, si = ko.cpu().numpy().view(R.wdtype(kind)), io.cpu().numpy().view(np.uint32)
        for k in (1, cols // 3, cols, np.array([7, C, 2 * C + 1, cols - 1])):
            gk, gi = run(ls, torch, x, k, largest, kind)
            ks = K.ks_of(k, rows)
            np.testing.assert_array_equal(gk, sk[np.arange(rows), ks - 1])
            np.testing.assert_array_equal(gi, si[np.arange(rows), ks - 1])


def test_one_workspace_reused(ls, torch_gpu):
    """Calls that mix key types, directions, paths and shapes on one workspace, never cleared between
    them; a call with a bad k in between does not leak into the next one's status."""
    torch = torch_gpu
    seq = [("bf16", 2, 70001), ("i32", 5, 300), ("f32", 3, 2 * C + 1), ("f16", 2, 16385), ("u32", 2, 70001),
           ("bf16", 3, 4097), ("f32", 2, 70001)]
    ws = torch.full((max(ls.kth_workspace_bytes(r, c) for _, r, c in seq),), 0xFF, dtype=torch.uint8, device="cuda")
    for i, (kind, rows, cols) in enumerate(seq):
        x, exp = R.case(kind, rows, cols)
        largest = bool(i & 1)
        if i == 2:
            run(ls, torch, x, np.array([0, 5, cols]), largest, kind, ws=ws, status=ls.ERR_ARG)
        check(ls, torch, x, cols // 2, largest, kind, exp=exp[largest], ws=ws, with_idx=i != 4)
        check(ls, torch, x, np.arange(1, rows + 1) * (cols // rows), not largest, kind, exp=exp[not largest], ws=ws)


@KINDS
def test_keys_only(ls, torch_gpu, kind):
    """d_idx_out = None writes the same keys and no position anywhere (run() checks the whole
    position storage), on both paths."""
    for rows, cols in ((3, 4097), (2, 70001)):
        x, exp = R.case(kind, rows, cols)
        for largest in BOTH:
            k1, _ = check(ls, torch_gpu, x, cols // 2, largest, kind, exp=exp[largest], with_idx=True)
            k0, _ = check(ls, torch_gpu, x, cols // 2, largest, kind, exp=exp[largest], with_idx=False)
            np.testing.assert_array_equal(k1, k0)


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
    ko = torch.zeros((rows,), dtype=sd, device="cuda")
    io = torch.zeros((rows,), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.kth_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.kth_device(src, rows, cols, dk, ko, io, largest=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.kth_device(src, rows, cols, dk, ko, io, largest=True, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    inputs = {"random": R.random_words((rows, cols), 0x4B18, kind), "ties": R.tie_words((rows, cols), 0x4B19, kind),
              "all_nan": np.full((rows, cols), R.nan_word(kind), dtype=R.wdtype(kind)),
              "planted": R.planted_words((rows, cols), 0x4B1A, kind)}
    rng = np.random.default_rng(0x4B1B)
    for dist, x in inputs.items():
        x = np.ascontiguousarray(x, dtype=R.wdtype(kind))
        ks = rng.integers(1, cols + 1, size=rows)
        src.copy_(to_dev(torch, x, kind))
        dk.copy_(torch.from_numpy(ks.astype(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.kth_workspace_status(ws)
        ek, ei = K.by_partition(x, ks, True, kind)
        K.assert_result(ko.cpu().numpy().view(R.wdtype(kind)), io.cpu().numpy().view(np.uint32), ek, ei, kind, dist)


SWEEP_SEEDS = (111, 112, 113)
SWEEP_CASES = 40


def sweep_cases(seed):
    """SWEEP_CASES cases: cols log-uniform in [1, 2^18], a third of the cases on m C + {-1, 0, 1};
    1 .. 6 rows; every kind; every row from its own generator (sort_sweep_model.sweep_row); direction
    and positions random; half of the cases with a random k per row, the others with one k."""
    for i in range(SWEEP_CASES):
        rng = np.random.default_rng([seed, 0x4B7A, i])
        if i % 3 == 0:
            cols = min(max(int(rng.integers(1, 17)) * C + int(rng.integers(-1, 2)), 1), 1 << 18)
        else:
            cols = min(max(int(np.exp(rng.uniform(0.0, np.log(1 << 18)))), 1), 1 << 18)
        rows = int(rng.integers(1, 7))
        kind = R.KINDS[int(rng.integers(0, len(R.KINDS)))]
        largest, with_idx = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        in_off = int(rng.integers(0, 2)) if R.is16(kind) else 0
        gens = [S.pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([S.sweep_row(g, cols, kind, largest, rng) for g in gens]).astype(R.wdtype(kind))
        k = rng.integers(1, cols + 1, size=rows) if i % 2 else int(rng.integers(1, cols + 1))
        tag = f"seed={seed} case={i} {kind} ({rows}, {cols}) k={k} largest={largest} idx={with_idx} in_off={in_off} rows={gens}"
        yield dict(x=x, k=k, kind=kind, largest=largest, with_idx=with_idx, in_off=in_off, tag=tag)


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_seeded_sweep(ls, torch_gpu, seed):
    """One workspace per seed, filled with 0xFF once and never cleared between the cases."""
    torch = torch_gpu
    cases = list(sweep_cases(seed))
    assert len(cases) == SWEEP_CASES
    ws = torch.full((max(ls.kth_workspace_bytes(*c["x"].shape) for c in cases),), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths = [], {"short": 0, "long": 0}
    for c in cases:
        paths["short" if c["x"].shape[1] <= ls.kth_row_keys() else "long"] += 1
        try:
            check(ls, torch, c["x"], c["k"], c["largest"], c["kind"], with_idx=c["with_idx"], in_off=c["in_off"], ws=ws)
        except AssertionError as err:
            failures.append(f"{c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {seed}: {paths}")
    assert paths["short"] >= 5 and paths["long"] >= 5
    assert not failures, failures


@pytest.mark.parametrize("kind", ["i32", "f32", "bf16", "f16"])
def test_python_kthvalue(ls, torch_gpu, kind):
    """ls.kthvalue on a (3, 70001) tensor, on a (4, 1000) one and on a 1-D tensor: shapes, dtypes,
    values, positions, an int k and a tensor k, the lower median, and the TypeErrors."""
    torch = torch_gpu
    tdt = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]
    for rows, cols in ((3, 70001), (4, 1000)):
        x, exp = R.case(kind, rows, cols)
        tg = to_dev(torch, x, kind).cuda().view(tdt)
        assert tg.shape == (rows, cols)
        med = (cols + 1) // 2
        v, i = ls.kthvalue(tg, med)
        assert v.dtype == tdt and i.dtype == torch.int32 and v.shape == (rows,) and i.shape == (rows,)
        ek, ei = K.by_sort(x, med, False, kind)
        K.assert_result(v.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), i.cpu().numpy().view(np.uint32), ek, ei, kind)
        ks = np.arange(1, rows + 1) * (cols // rows)
        kt = torch.from_numpy(ks.astype(np.int32)).cuda()
        v, i = ls.kthvalue(tg, kt, largest=True)
        ek, ei = K.by_sort(x, ks, True, kind)
        K.assert_result(v.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), i.cpu().numpy().view(np.uint32), ek, ei, kind)
        row = tg[1].contiguous()  # 1-D: one row
        v, i = ls.kthvalue(row, 5, largest=True)
        assert v.shape == (1,) and i.shape == (1,) and v.dtype == tdt
        ek, ei = K.by_sort(x[1:2], 5, True, kind)
        K.assert_result(v.view(sdtype(torch, kind)).cpu().numpy().view(R.wdtype(kind)), i.cpu().numpy().view(np.uint32), ek, ei, kind)
        for badk in (kt.to(torch.int64), kt[:2], kt.cpu(), torch.stack([kt, kt], dim=1)[:, 0], kt.view(1, rows), 2.5, "3", None):
            with pytest.raises(TypeError):
                ls.kthvalue(tg, badk)
        with pytest.raises(TypeError):
            ls.kthvalue(tg.t(), 1)
        with pytest.raises(ls.LabsortError):
            ls.kthvalue(tg, cols + 1)  # the host k is checked before any launch
        with pytest.raises(ls.LabsortError) as e:
            ls.kthvalue(tg, torch.zeros(rows, dtype=torch.int32, device="cuda"))  # a device k: reported by the status
        assert e.value.status == ls.ERR_ARG
