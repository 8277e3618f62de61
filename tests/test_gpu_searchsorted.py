"""GPU tests of labsort_searchsorted_device / ls.searchsorted_device / ls.searchsorted / ls.bucketize
against the numpy model (tests/searchsorted_model.py): every rank compared word for word, canaries in
front of and behind d_out, the inputs unchanged.  L = ls.searchsorted_row_keys(kind) is the longest
sequence of the LDS path, V = ls.searchsorted_chunk_values() the values of a workgroup step; the
workspace of every call is filled with garbage first."""
import numpy as np
import pytest

import searchsorted_model as SM

pytestmark = pytest.mark.gpu

GUARD = 64  # canary words on each side of the output
S = np.uint32(SM.SENTINEL)
ALL = pytest.mark.parametrize("kind", SM.KINDS)


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def run(ls, torch, seq, vals, right, kind, sorter=None, want=None, off=0, tag=""):
    """One searchsorted_device call, checked against `want` (None: only that every rank lies in
    [0, cols]).  seq: 1-D (one sequence for every value) or rows x cols; vals: 1-D or rows x nv.  off:
    sequence, sorter, values and output start that many elements into their buffers."""
    dt, e = SM.word_dtype(kind), SM.esz(kind)
    seq, vals = np.ascontiguousarray(seq, dtype=dt), np.ascontiguousarray(vals, dtype=dt)
    seq_rows, cols = (1, seq.size) if seq.ndim == 1 else seq.shape
    rows, nv = (1, vals.size) if vals.ndim == 1 else vals.shape
    msg = f"{tag} {kind} cols={cols} seq_rows={seq_rows} rows={rows} nv={nv} right={right} off={off} sorter={sorter is not None}"
    lead = lambda a: np.concatenate([np.full(off, 0x5A, dtype=a.dtype), a.reshape(-1)])  # noqa: E731
    h_seq, h_vals = lead(seq), lead(vals)
    d_seq, d_vals = to_dev(torch, h_seq), to_dev(torch, h_vals)
    h_sorter = d_sorter = None
    if sorter is not None:
        h_sorter = lead(np.ascontiguousarray(sorter, dtype=np.uint32))
        d_sorter = to_dev(torch, h_sorter)
    n = rows * nv
    d_out = to_dev(torch, np.full(GUARD + off + n + GUARD, S, dtype=np.uint32))
    need = ls.searchsorted_workspace_bytes(seq_rows, cols, kind)
    assert (need == 0) == (cols <= ls.searchsorted_row_keys(kind)), msg
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda") if need else None
    ls.searchsorted_device(d_seq.data_ptr() + off * e if cols else None, seq_rows, cols, d_vals.data_ptr() + off * e, rows, nv,
                           d_out.data_ptr() + (GUARD + off) * 4, right=right, key=kind,
                           d_sorter=None if d_sorter is None else d_sorter.data_ptr() + off * 4, workspace=ws)
    torch.cuda.synchronize()
    host = lambda t, d: t.cpu().numpy().view(d)  # noqa: E731
    out = host(d_out, np.uint32)
    got = out[GUARD + off:GUARD + off + n].reshape(vals.shape)
    assert bool((out[:GUARD + off] == S).all()) and bool((out[GUARD + off + n:] == S).all()), f"canaries: {msg}"
    if want is None:
        assert int(got.max()) <= cols, f"rank past cols: {msg}"
    else:
        np.testing.assert_array_equal(got, want, err_msg=msg)
    np.testing.assert_array_equal(host(d_seq, dt), h_seq, err_msg=f"the sequence was written: {msg}")
    np.testing.assert_array_equal(host(d_vals, dt), h_vals, err_msg=f"the values were written: {msg}")
    if d_sorter is not None:
        np.testing.assert_array_equal(host(d_sorter, np.uint32), h_sorter, err_msg=f"the sorter was written: {msg}")
    return got


def LV(ls, kind):
    return ls.searchsorted_row_keys(kind), ls.searchsorted_chunk_values()


def stride_of(cols):
    return (cols + SM.SAMPLES - 1) // SM.SAMPLES


# ---- sizes -----------------------------------------------------------------------------------------
COLS_IDS = ["0", "1", "2", "3", "63", "64", "65", "L-1", "L", "L+1", "4096k-1", "4096k", "4096k+1", "4096(k+1)-1", "4096(k+1)",
            "4096(k+1)+1", "3*2^20+5"]


@ALL
@pytest.mark.parametrize("cid", COLS_IDS)
def test_cols_sizes(ls, torch_gpu, cid, kind):
    """Every sequence length at which the entry takes another path, another stride or another number
    of probes, with values around the sequence's elements: one shared sequence with both sides, and
    a sequence per row (3 rows; 1 at the longest).  Each length takes another nv of nv_sizes."""
    L, V = LV(ls, kind)
    i = COLS_IDS.index(cid)
    cols = SM.cols_sizes(L)[i]
    nvs = SM.nv_sizes(V)
    nv = nvs[i % len(nvs)]
    seq, vals, left, right = SM.shared_case("random", cols, nv, 0x5E0 + i, kind)
    run(ls, torch_gpu, seq, vals, False, kind, want=left, tag=cid)
    run(ls, torch_gpu, seq, vals, True, kind, want=right, tag=cid)
    rows = 1 if cid == COLS_IDS[-1] else 3
    seq, vals, left, right = SM.row_case("random", rows, cols, nvs[(i + 3) % len(nvs)], 0x5E0 + i, kind)
    run(ls, torch_gpu, seq, vals, bool(i & 1), kind, want=right if i & 1 else left, tag=cid + " per row")


NV_IDS = ["1", "7", "8", "9", "V-1", "V", "V+1", "3V+5"]


@ALL
@pytest.mark.parametrize("nid", NV_IDS)
def test_nv_sizes(ls, torch_gpu, nid, kind):
    """Every nv around the 16-byte group and the chunk, in both forms and on both paths: one sequence
    with one row and with 3 rows of values, a sequence per row with 1, 3 and 257 rows (5 rows at
    3V + 5, where 257 would be three million values)."""
    L, V = LV(ls, kind)
    i = NV_IDS.index(nid)
    nv = SM.nv_sizes(V)[i]
    for cols in (65, L + 1):
        seq, vals, left, right = SM.shared_case("random", cols, nv, 0x7A0 + i, kind)
        run(ls, torch_gpu, seq, vals, False, kind, want=left, tag=nid)
        run(ls, torch_gpu, seq, vals, True, kind, want=right, tag=nid)
        v3 = np.stack([vals, vals[::-1], np.roll(vals, 3)])
        run(ls, torch_gpu, seq, v3, True, kind, want=np.stack([right, right[::-1], np.roll(right, 3)]), tag=nid + " 3 rows, shared")
    for rows, cols in ((1, 64), (3, L + 1), (257 if nv <= V + 1 else 5, 63), (3, L)):
        seq, vals, left, right = SM.row_case("random", rows, cols, nv, 0x7B0 + i, kind)
        side = bool((i + rows) & 1)
        run(ls, torch_gpu, seq, vals, side, kind, want=right if side else left, tag=f"{nid} per row")


@pytest.mark.parametrize("kind", ["u32", "bf16", "f64"])
def test_257_rows_long_path(ls, torch_gpu, kind):
    L, V = LV(ls, kind)
    seq, vals, left, right = SM.row_case("few", 257, L + 1, 9, 0x257, kind)
    run(ls, torch_gpu, seq, vals, False, kind, want=left)
    run(ls, torch_gpu, seq, vals, True, kind, want=right)


# ---- run shapes --------------------------------------------------------------------------------------
@ALL
@pytest.mark.parametrize("path", ["lds", "long"])
def test_run_shapes(ls, torch_gpu, path, kind):
    """All keys equal, two distinct keys, few keys in long runs; on the long path runs of stride - 1,
    stride + 1 and 3 strides + 5 elements, so that consecutive samples of the table tie and both
    sides must still land on the run's two ends."""
    L, V = LV(ls, kind)
    cols = 3 * L + 77 if path == "long" else L - 3
    st = stride_of(cols)
    gens = ["equal", "two", "few"] + ([f"runs:{st - 1}", f"runs:{st + 1}", f"runs:{3 * st + 5}"] if path == "long" else ["runs:5"])
    for gen in gens:
        seq, vals, left, right = SM.shared_case(gen, cols, V + 9, 0x8C0, kind)
        run(ls, torch_gpu, seq, vals, False, kind, want=left, tag=gen)
        run(ls, torch_gpu, seq, vals, True, kind, want=right, tag=gen)


@pytest.mark.parametrize("kind", ["u64", "i64"])
@pytest.mark.parametrize("which", ["lo", "hi"])
def test_64_bit_halves(ls, torch_gpu, which, kind):
    """Keys that differ in the low half only (all above 2^63) and in the high half only."""
    L, V = LV(ls, kind)
    for cols in (L - 1, 2 * L + 3):
        raw = SM.half_words(cols, 0x64, which)
        seq = SM.ascending(raw, kind)
        vals = SM.probes(seq, kind)[::3][:2 * V + 1]
        for right in (False, True):
            run(ls, torch_gpu, seq, vals, right, kind, want=SM.expected(seq, vals, right, kind), tag=which)


@pytest.mark.parametrize("kind", SM.FLOATS)
def test_float_specials_in_sequence_and_values(ls, torch_gpu, kind):
    """NaNs of several payloads and signs, both zeros, both infinities: several of each in the sequence,
    each one a value."""
    L, V = LV(ls, kind)
    s = SM.float_specials(kind)
    for cols in (3 * s.size, L + 100):
        raw = np.concatenate([np.tile(s, 3), SM.random_words(cols - 3 * s.size, 0xF10A, kind)])
        seq = SM.ascending(raw, kind)
        vals = np.concatenate([s, SM.probes(s, kind)])
        for right in (False, True):
            run(ls, torch_gpu, seq, vals, right, kind, want=SM.expected(seq, vals, right, kind))


# ---- sorter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u32", "f32", "i64", "f16"])
@pytest.mark.parametrize("path", ["lds", "long"])
def test_sorter(ls, torch_gpu, path, kind):
    """A random permutation of a sorted row with the sorter that undoes it: one sequence and three."""
    L, V = LV(ls, kind)
    cols = 2 * L + 5 if path == "long" else L
    rng = np.random.default_rng(0x50A7)
    rows = []
    for r in range(3):
        seq = SM.sequence("few" if r == 1 else "random", cols, 0x50A0 + r, kind)
        perm = rng.permutation(cols)
        raw = np.empty_like(seq)
        raw[perm] = seq  # raw[perm[i]] = seq[i]
        rows.append((raw, perm.astype(np.uint32), SM.probes(seq, kind)[::5][:V + 3]))
    for right in (False, True):
        raw, perm, vals = rows[0]
        run(ls, torch_gpu, raw, vals, right, kind, sorter=perm, want=SM.expected(raw, vals, right, kind, perm))
    raw, perm = np.stack([t[0] for t in rows]), np.stack([t[1] for t in rows])
    nv = min(t[2].size for t in rows)
    vals = np.stack([t[2][:nv] for t in rows])
    run(ls, torch_gpu, raw, vals, True, kind, sorter=perm, want=SM.expected(raw, vals, True, kind, perm))


@pytest.mark.parametrize("kind", ["i32", "u64"])
@pytest.mark.parametrize("path", ["lds", "long"])
def test_sorter_entries_past_the_row(ls, torch_gpu, path, kind):
    """A caller error: the kernels clamp such an entry, so ranks stay in range and nothing is read or
    written out of bounds."""
    L, V = LV(ls, kind)
    cols = L + 4097 if path == "long" else 1000
    rng = np.random.default_rng(0xBAD)
    seq = SM.sequence("random", cols, 0xBAD, kind)
    sorter = np.arange(cols, dtype=np.uint32)
    at = rng.integers(0, cols, size=cols // 3)
    sorter[at] = rng.choice(np.array([cols, cols + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), size=at.size)
    sorter[-1] = 0xFFFFFFFF
    for right in (False, True):
        run(ls, torch_gpu, seq, SM.probes(seq, kind)[:2 * V + 7], right, kind, sorter=sorter, want=None)


# ---- an unsorted sequence ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u32", "f16", "f64"])
@pytest.mark.parametrize("path", ["lds", "long"])
def test_unsorted_sequence(ls, torch_gpu, path, kind):
    """Random keys as they fall: the ranks are unspecified but lie in [0, cols], the canaries hold and
    the call returns."""
    L, V = LV(ls, kind)
    cols = 3 * L + 11 if path == "long" else L - 1
    raw = SM.random_words(cols, 0x0BAD5EED, kind)
    vals = np.concatenate([raw[:V], SM.random_words(V + 5, 7, kind)])
    for right in (False, True):
        run(ls, torch_gpu, raw, vals, right, kind, want=None)
        run(ls, torch_gpu, np.stack([raw, raw[::-1]]), np.stack([vals, vals]), right, kind, want=None)


# ---- unaligned views ---------------------------------------------------------------------------------
@ALL
@pytest.mark.parametrize("off", [1, 3])
def test_unaligned_views(ls, torch_gpu, off, kind):
    """Sequence, values and output start 1 and 3 elements into their buffers, on both paths; with a
    sequence per row and odd cols and nv the rows start at every alignment."""
    L, V = LV(ls, kind)
    for cols in (L - 5, L + 5):
        seq, vals, left, right = SM.shared_case("random", cols, V + 11, 0xA11, kind)
        run(ls, torch_gpu, seq, vals, False, kind, want=left, off=off)
        run(ls, torch_gpu, seq, vals, True, kind, want=right, off=off)
    for cols in (1001, L + 7):
        seq, vals, left, right = SM.row_case("random", 5, cols, 2 * V + 3, 0xA12, kind)
        run(ls, torch_gpu, seq, vals, True, kind, want=right, off=off)


# ---- seeded sweep --------------------------------------------------------------------------------------
def test_seeded_sweep(ls, torch_gpu):
    """40 cases over key type, path, form, side and sorter, rows and values from the generators of
    tests/sort_sweep_model.py."""
    row_keys = {k: ls.searchsorted_row_keys(k) for k in SM.KINDS}
    cases = list(SM.sweep_cases(0x5EA, row_keys, ls.searchsorted_chunk_values()))
    assert len(cases) == 40
    for c in cases:
        seq, vals, sorter, want = SM.sweep_case(c)
        run(ls, torch_gpu, seq, vals, c["right"], c["kind"], sorter=sorter, want=want, tag=c["tag"])


# ---- graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,path", [("f32", "lds"), ("i64", "long"), ("bf16", "long")])
def test_graph_replay(ls, torch_gpu, kind, path):
    """One call captured on a side stream and replayed on three new (sequence, values) sets in the same
    buffers: the launch sequence depends on the host arguments only."""
    torch = torch_gpu
    L, V = LV(ls, kind)
    cols, nv, rows = (2 * L + 9 if path == "long" else L - 7), V + 5, 3
    e = SM.esz(kind)
    d_seq = torch.zeros(rows * cols * e, dtype=torch.uint8, device="cuda")
    d_vals = torch.zeros(rows * nv * e, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(rows * nv, dtype=torch.int32, device="cuda")
    need = ls.searchsorted_workspace_bytes(rows, cols, kind)
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda") if need else None
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.searchsorted_device(d_seq, rows, cols, d_vals, rows, nv, d_out, right=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.searchsorted_device(d_seq, rows, cols, d_vals, rows, nv, d_out, right=True, key=kind, workspace=ws,
                               stream=torch.cuda.current_stream())
    for j, gen in enumerate(("random", "few", "two")):
        seq, vals, _, want = SM.row_case(gen, rows, cols, nv, 0x6A0 + j, kind)
        d_seq.copy_(to_dev(torch, seq))
        d_vals.copy_(to_dev(torch, vals))
        d_out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint32).reshape(rows, nv), want, err_msg=f"replay {gen} {kind}")


# ---- ls.searchsorted / ls.bucketize --------------------------------------------------------------------
def torch_keys(torch, kind, shape, seed, lo=-1000, hi=1000):
    """NaN-free keys without zeros (torch compares floats as the hardware does)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind in ("i32", "i64"):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32 if kind == "i32" else torch.int64).cuda()
    x = torch.randn(shape, generator=g, dtype=torch.float32 if kind == "f32" else torch.float64) * 50
    return torch.where(x == 0, torch.ones_like(x), x).cuda()


@pytest.mark.parametrize("kind", ["i32", "f32", "i64", "f64"])
def test_wrappers_against_torch(ls, torch_gpu, kind):
    """ls.searchsorted / ls.bucketize against torch.searchsorted(out_int32=True) / torch.bucketize: 1-D
    and batched, with and without a sorter, both sides and both ways to name the side, both paths."""
    torch = torch_gpu
    L, V = LV(ls, kind)
    for cols in (777, L + 3):
        raw = torch_keys(torch, kind, (3, cols), 0x70 + cols)
        seq, order = torch.sort(raw, dim=-1, stable=True)
        vals = torch.cat([torch_keys(torch, kind, (3, V + 5), 0x71), raw[:, :100]], dim=-1).contiguous()
        for right in (False, True):
            side = "right" if right else "left"
            want = torch.searchsorted(seq, vals, out_int32=True, right=right)
            got = ls.searchsorted(seq, vals, right=right)
            assert got.dtype == torch.int32 and got.shape == vals.shape and torch.equal(got, want)
            assert torch.equal(ls.searchsorted(seq, vals, side=side), want)
            assert torch.equal(ls.searchsorted(raw, vals, side=side, sorter=order.int()), want)
            assert torch.equal(want, torch.searchsorted(raw, vals, out_int32=True, side=side, sorter=order))
            # a 1-D sequence with values of any shape
            want1 = torch.searchsorted(seq[1], vals, out_int32=True, right=right)
            assert torch.equal(ls.searchsorted(seq[1], vals, right=right), want1)
            assert torch.equal(ls.searchsorted(raw[1].contiguous(), vals, right=right, sorter=order[1].int().contiguous()), want1)
            assert torch.equal(ls.bucketize(vals, seq[1], right=right), torch.bucketize(vals, seq[1], out_int32=True, right=right))
            v3 = vals[:, :35].reshape(3, 5, 7).contiguous()
            assert torch.equal(ls.bucketize(v3, seq[2], right=right), torch.bucketize(v3, seq[2], out_int32=True, right=right))
    # empty ends
    seq = torch_keys(torch, kind, (50,), 5).sort().values
    assert ls.searchsorted(seq, seq[:0]).shape == (0,)
    assert torch.equal(ls.searchsorted(seq[:0], seq), torch.zeros(50, dtype=torch.int32, device="cuda"))
    assert torch.equal(ls.searchsorted(seq[:0], seq, right=True), torch.searchsorted(seq[:0], seq, out_int32=True, right=True))


@pytest.mark.parametrize("kind", ["bf16", "f16", "u32", "u64", "f32", "f64"])
def test_wrappers_against_the_model(ls, torch_gpu, kind):
    """The dtypes torch.searchsorted does not take (and, for float32 and float64, the NaNs and zeros
    on which it differs) against the model."""
    torch = torch_gpu
    L, V = LV(ls, kind)
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "u32": torch.uint32, "u64": torch.uint64, "f32": torch.float32,
           "f64": torch.float64}[kind]
    signed = {2: np.int16, 4: np.int32, 8: np.int64}[SM.esz(kind)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).cuda().view(tdt)  # noqa: E731
    for cols in (500, L + 9):
        seq, vals, left, right = SM.row_case("random", 2, cols, V + 3, 0x90D, kind)
        for r, want in ((False, left), (True, right)):
            got = ls.searchsorted(dev(seq), dev(vals), right=r)
            assert got.dtype == torch.int32
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want, err_msg=f"{kind} cols={cols} right={r}")
            got = ls.bucketize(dev(vals), dev(seq[0]), right=r)
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), SM.expected(seq[0], vals, r, kind))
        perm = np.random.default_rng(3).permutation(cols)
        raw = np.empty_like(seq[1])
        raw[perm] = seq[1]
        got = ls.searchsorted(dev(raw), dev(vals[1]), side="right", sorter=torch.from_numpy(perm.astype(np.int32)).cuda())
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), right[1])
