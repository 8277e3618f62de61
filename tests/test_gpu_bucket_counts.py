"""GPU tests of labsort_bucket_counts_device / labsort_bincount_device and their Python wrappers
against the numpy models (tests/bucket_counts_model.py, built on tests/searchsorted_model.py): every
count compared word for word, canaries in front of and behind d_counts_out, the inputs unchanged, the
output and the workspace of every call filled with garbage first.  E = ls.bucket_counts_row_edges(kind)
is the longest edge row of the LDS path, V = ls.searchsorted_chunk_values() the values of a workgroup
step.

Every counter of the kernels, in LDS and in global memory, is a 32-bit word and rows * nv <= 2^31 - 1,
so no counter can overflow: there is no narrower counter to test."""
import numpy as np
import pytest

import bucket_counts_model as BM
import searchsorted_model as SM

pytestmark = pytest.mark.gpu

GUARD = 64  # canary words on each side of the output
S = np.uint32(SM.SENTINEL)
ALL = pytest.mark.parametrize("kind", SM.KINDS)
PATHS = pytest.mark.parametrize("path", ["lds", "long"])


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def host(t, d):
    return t.cpu().numpy().view(d)


def check_out(out, off, n, msg):
    assert bool((out[:GUARD + off] == S).all()) and bool((out[GUARD + off + n:] == S).all()), f"canaries: {msg}"
    return out[GUARD + off:GUARD + off + n]


def run(ls, torch, edges, vals, right, kind, want=None, off=0, tag=""):
    """One bucket_counts_device call, checked against `want` (None: only that every row sums to nv).
    edges: 1-D (one edge row for every row of the values) or rows x nedges; vals: 1-D or rows x nv.
    off: edges, values and output start that many elements into their buffers."""
    dt, e = SM.word_dtype(kind), SM.esz(kind)
    edges, vals = np.ascontiguousarray(edges, dtype=dt), np.ascontiguousarray(vals, dtype=dt)
    edge_rows, nedges = (1, edges.size) if edges.ndim == 1 else edges.shape
    rows, nv = (1, vals.size) if vals.ndim == 1 else vals.shape
    msg = f"{tag} {kind} nedges={nedges} edge_rows={edge_rows} rows={rows} nv={nv} right={right} off={off}"
    lead = lambda a: np.concatenate([np.full(off, 0x5A, dtype=a.dtype), a.reshape(-1)])  # noqa: E731
    h_edges, h_vals = lead(edges), lead(vals)
    d_edges, d_vals = to_dev(torch, h_edges), to_dev(torch, h_vals)
    n = rows * (nedges + 1)
    d_out = to_dev(torch, np.full(GUARD + off + n + GUARD, S, dtype=np.uint32))
    need = ls.bucket_counts_workspace_bytes(edge_rows, nedges, kind)
    assert (need == 0) == (nedges <= ls.bucket_counts_row_edges(kind)), msg
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda") if need else None
    ls.bucket_counts_device(d_edges.data_ptr() + off * e if nedges else None, edge_rows, nedges,
                            d_vals.data_ptr() + off * e if nv else None, rows, nv, d_out.data_ptr() + (GUARD + off) * 4,
                            right=right, key=kind, workspace=ws)
    torch.cuda.synchronize()
    got = check_out(host(d_out, np.uint32), off, n, msg).reshape(rows, nedges + 1)
    if want is not None:
        np.testing.assert_array_equal(got, np.asarray(want).reshape(rows, nedges + 1), err_msg=msg)
    np.testing.assert_array_equal(got.sum(axis=1, dtype=np.uint64), np.full(rows, nv, dtype=np.uint64), err_msg=f"row sums: {msg}")
    np.testing.assert_array_equal(host(d_edges, dt), h_edges, err_msg=f"the edges were written: {msg}")
    np.testing.assert_array_equal(host(d_vals, dt), h_vals, err_msg=f"the values were written: {msg}")
    return got


def both_sides(ls, torch, edges, vals, kind, left, right, **kw):
    """ranks left / right of the values (tests/searchsorted_model.py's cases carry them) -> both calls"""
    nedges = np.asarray(edges).shape[-1]
    run(ls, torch, edges, vals, False, kind, want=BM.counts_of_ranks(left, nedges), **kw)
    run(ls, torch, edges, vals, True, kind, want=BM.counts_of_ranks(right, nedges), **kw)


def EV(ls, kind):
    return ls.bucket_counts_row_edges(kind), ls.searchsorted_chunk_values()


def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- sizes -----------------------------------------------------------------------------------------
NEDGES_IDS = ["0", "1", "2", "3", "63", "64", "65", "E-1", "E", "E+1", "4096k-1", "4096k", "4096k+1", "4096(k+1)-1", "4096(k+1)",
              "4096(k+1)+1", "3*2^20+5"]


@ALL
@pytest.mark.parametrize("cid", NEDGES_IDS)
def test_nedges_sizes(ls, torch_gpu, cid, kind):
    """Every number of edges at which the entry takes another path, another stride or another number
    of probes, with values around the edges: one shared edge row with 3 rows of values and an edge
    row per row (3 rows; 1 at the longest), both sides.  Each length takes another nv of nv_sizes."""
    E, V = EV(ls, kind)
    i = NEDGES_IDS.index(cid)
    nedges = SM.cols_sizes(E)[i]
    nvs = SM.nv_sizes(V)
    nv = nvs[i % len(nvs)]
    edges, vals, left, right = SM.shared_case("random", nedges, nv, 0x5E0 + i, kind)
    three = lambda a: np.stack([a, a[::-1], np.roll(a, 3)])  # noqa: E731
    both_sides(ls, torch_gpu, edges, three(vals), kind, three(left), three(right), tag=cid + " shared")
    rows = 1 if cid == NEDGES_IDS[-1] else 3
    edges, vals, left, right = SM.row_case("random", rows, nedges, nvs[(i + 3) % len(nvs)], 0x5E0 + i, kind)
    both_sides(ls, torch_gpu, edges, vals, kind, left, right, tag=cid + " per row")


NV_IDS = ["1", "7", "8", "9", "V-1", "V", "V+1", "3V+5"]


@ALL
@pytest.mark.parametrize("nid", NV_IDS)
def test_nv_sizes(ls, torch_gpu, nid, kind):
    """Every nv around the 16-byte group and the chunk on both paths: a shared edge row with 1, 3 and
    257 rows of values, an edge row per row with 1, 3 and 257 rows (5 rows instead of 257 at 3V + 5,
    where 257 would be three million values).  At 3V + 5 a row has several workgroups, which add
    their counters to the output with atomics; below that one workgroup stores them."""
    E, V = EV(ls, kind)
    i = NV_IDS.index(nid)
    nv = SM.nv_sizes(V)[i]
    many = 257 if nv <= V + 1 else 5
    for nedges in (65, E + 1):
        edges, vals, left, right = SM.shared_case("random", nedges, nv, 0x7A0 + i, kind)
        both_sides(ls, torch_gpu, edges, vals, kind, left, right, tag=nid)
        three = lambda a: np.stack([a, a[::-1], np.roll(a, 3)])  # noqa: E731
        run(ls, torch_gpu, edges, three(vals), True, kind, want=BM.counts_of_ranks(three(right), nedges), tag=nid + " 3 rows, shared")
        if nedges == 65:
            rolled = lambda a: np.stack([np.roll(a, r) for r in range(many)])  # noqa: E731
            run(ls, torch_gpu, edges, rolled(vals), False, kind, want=BM.counts_of_ranks(rolled(left), nedges), tag=f"{nid} {many} rows, shared")
    for rows, nedges in ((1, 64), (3, E + 1), (many, 63), (3, E)):
        edges, vals, left, right = SM.row_case("random", rows, nedges, nv, 0x7B0 + i, kind)
        side = bool((i + rows) & 1)
        run(ls, torch_gpu, edges, vals, side, kind, want=BM.counts_of_ranks(right if side else left, nedges), tag=f"{nid} per row")


@pytest.mark.parametrize("kind", ["u32", "bf16", "f64"])
def test_257_rows_long_path(ls, torch_gpu, kind):
    E, V = EV(ls, kind)
    edges, vals, left, right = SM.row_case("few", 257, E + 1, 9, 0x257, kind)
    both_sides(ls, torch_gpu, edges, vals, kind, left, right)


@pytest.mark.parametrize("kind", ["f32", "i64"])
def test_no_values(ls, torch_gpu, kind):
    """nv == 0 writes zeros over whatever the output held, on both paths and in both forms."""
    E, V = EV(ls, kind)
    for nedges in (0, 77, E + 1):
        edges = SM.sequence("random", nedges, 0xE0, kind)
        for rows in (1, 3):
            got = run(ls, torch_gpu, edges, np.zeros((rows, 0), dtype=SM.word_dtype(kind)), False, kind,
                      want=np.zeros((rows, nedges + 1), dtype=np.uint32))
            assert got.shape == (rows, nedges + 1)
        run(ls, torch_gpu, np.stack([edges] * 3), np.zeros((3, 0), dtype=SM.word_dtype(kind)), True, kind,
            want=np.zeros((3, nedges + 1), dtype=np.uint32))


# ---- geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u32", "bf16"])
@PATHS
def test_more_chunks_than_workgroups(ls, torch_gpu, path, kind):
    """One row on a shared edge row with more chunks than the grid has workgroups (two per CU on the
    LDS path, four on the long one): every workgroup takes several chunks and all of them add to the
    one row of counters."""
    E, V = EV(ls, kind)
    nv = (4 * cus(torch_gpu) + 3) * V + 5
    nedges = E + 1 if path == "long" else 1000
    edges, vals, left, right = SM.shared_case("random", nedges, nv, 0x6E0, kind)
    both_sides(ls, torch_gpu, edges, vals, kind, left, right, tag="chunks > grid")


# ---- skew ----------------------------------------------------------------------------------------------
@ALL
@PATHS
def test_skew(ls, torch_gpu, path, kind):
    """What makes many lanes hit one counter: all values equal, all below the first edge, all past the
    last one, all NaN, values already sorted; and edges with long runs of equal keys, which leave
    most bins empty.  One row of 2V + 9 values (two or three workgroups) and three rows."""
    E, V = EV(ls, kind)
    dt = SM.word_dtype(kind)
    nedges = 3 * E + 77 if path == "long" else E - 3
    nv = 2 * V + 9
    st = (nedges + SM.SAMPLES - 1) // SM.SAMPLES
    edges, drawn, _, _ = SM.shared_case("random", nedges, nv, 0x8C0, kind)
    top = np.iinfo(dt).max
    fills = {"equal": edges[nedges // 2], "first edge": edges[0], "last edge": edges[-1],
             "smallest": SM.from_image(np.array([0], dtype=dt), kind)[0], "largest (NaN)": SM.from_image(np.array([top], dtype=dt), kind)[0]}
    if kind in SM.FLOATS:
        fills["a special"] = SM.float_specials(kind)[-2]
    for name, word in fills.items():
        vals = np.full(nv, word, dtype=dt)
        for right in (False, True):
            got = run(ls, torch_gpu, edges, vals, right, kind, want=BM.expected(edges, vals, right, kind), tag=name)
            assert int(got.max()) == nv  # one bin holds them all
    in_order = SM.ascending(drawn, kind)
    for right in (False, True):
        run(ls, torch_gpu, edges, in_order, right, kind, want=BM.expected(edges, in_order, right, kind), tag="sorted values")
    rows3 = np.stack([in_order, np.full(nv, edges[0], dtype=dt), drawn])
    run(ls, torch_gpu, edges, rows3, False, kind, want=BM.expected(edges, rows3, False, kind), tag="3 rows")
    gens = ["equal", "two", "few"] + ([f"runs:{st - 1}", f"runs:{st + 1}", f"runs:{3 * st + 5}"] if path == "long" else ["runs:5"])
    for gen in gens:
        edges, vals, left, right = SM.shared_case(gen, nedges, V + 9, 0x8C0, kind)
        both_sides(ls, torch_gpu, edges, vals, kind, left, right, tag=gen)


@pytest.mark.parametrize("kind", SM.FLOATS)
def test_float_specials_in_edges_and_values(ls, torch_gpu, kind):
    """NaNs of several payloads and signs, both zeros, both infinities: several of each among the
    edges, each one a value."""
    E, V = EV(ls, kind)
    s = SM.float_specials(kind)
    for nedges in (3 * s.size, E + 100):
        raw = np.concatenate([np.tile(s, 3), SM.random_words(nedges - 3 * s.size, 0xF10A, kind)])
        edges = SM.ascending(raw, kind)
        vals = np.concatenate([s, SM.probes(s, kind)])
        for right in (False, True):
            run(ls, torch_gpu, edges, vals, right, kind, want=BM.expected(edges, vals, right, kind))


# ---- unsorted edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u32", "f16", "f64"])
@PATHS
def test_unsorted_edges(ls, torch_gpu, path, kind):
    """Random keys as they fall: the counts are unspecified but every row sums to nv, the canaries hold
    and the call returns."""
    E, V = EV(ls, kind)
    nedges = 3 * E + 11 if path == "long" else E - 1
    raw = SM.random_words(nedges, 0x0BAD5EED, kind)
    vals = np.concatenate([raw[:V], SM.random_words(V + 5, 7, kind)])
    for right in (False, True):
        run(ls, torch_gpu, raw, vals, right, kind, want=None)
        run(ls, torch_gpu, np.stack([raw, raw[::-1]]), np.stack([vals, vals]), right, kind, want=None)


# ---- unaligned views -----------------------------------------------------------------------------------
@ALL
@pytest.mark.parametrize("off", [1, 3])
def test_unaligned_views(ls, torch_gpu, off, kind):
    """Edges, values and output start 1 and 3 elements into their buffers, on both paths; with an edge
    row per row and odd nedges and nv the rows start at every alignment."""
    E, V = EV(ls, kind)
    for nedges in (E - 5, E + 5):
        edges, vals, left, right = SM.shared_case("random", nedges, V + 11, 0xA11, kind)
        both_sides(ls, torch_gpu, edges, vals, kind, left, right, off=off)
    for nedges in (1001, E + 7):
        edges, vals, left, right = SM.row_case("random", 5, nedges, 2 * V + 3, 0xA12, kind)
        run(ls, torch_gpu, edges, vals, True, kind, want=BM.counts_of_ranks(right, nedges), off=off)


# ---- seeded sweep --------------------------------------------------------------------------------------
def test_seeded_sweep(ls, torch_gpu):
    """40 cases over key type, path, form and side, rows and values from the generators of
    tests/sort_sweep_model.py (a case drawn with a sorter has its rows put in order here: this entry
    takes none)."""
    row_edges = {k: ls.bucket_counts_row_edges(k) for k in SM.KINDS}
    cases = list(SM.sweep_cases(0x5EA, row_edges, ls.searchsorted_chunk_values()))
    assert len(cases) == 40
    for c in cases:
        seq, vals, sorter, ranks = SM.sweep_case(c)
        if sorter is not None:
            seq = np.take_along_axis(seq, sorter.astype(np.int64), axis=-1)
        if seq.ndim == 1 and vals.shape[0] == 1:
            vals, ranks = vals[0], ranks[0]
        run(ls, torch_gpu, seq, vals, c["right"], c["kind"], want=BM.counts_of_ranks(ranks, c["cols"]), tag=c["tag"])


# ---- bincount ------------------------------------------------------------------------------------------
def run_bincount(ls, torch, vals, nbins, kind, off=0, tag=""):
    dt, e = SM.word_dtype(kind), SM.esz(kind)
    vals = np.ascontiguousarray(vals, dtype=dt)
    rows, nv = (1, vals.size) if vals.ndim == 1 else vals.shape
    msg = f"{tag} bincount {kind} nbins={nbins} rows={rows} nv={nv} off={off}"
    h_vals = np.concatenate([np.full(off, 0x5A, dtype=dt), vals.reshape(-1)])
    d_vals = to_dev(torch, h_vals)
    n = rows * (nbins + 1)
    d_out = to_dev(torch, np.full(GUARD + off + n + GUARD, S, dtype=np.uint32))
    ls.bincount_device(d_vals.data_ptr() + off * e if nv else None, rows, nv, nbins, d_out.data_ptr() + (GUARD + off) * 4, key=kind)
    torch.cuda.synchronize()
    got = check_out(host(d_out, np.uint32), off, n, msg).reshape(rows, nbins + 1)
    np.testing.assert_array_equal(got, BM.bincount_expected(vals, nbins, kind).reshape(rows, nbins + 1), err_msg=msg)
    np.testing.assert_array_equal(host(d_vals, dt), h_vals, err_msg=f"the values were written: {msg}")
    return got


BIN_IDS = ["0", "1", "255", "256", "B", "B+1"]


@pytest.mark.parametrize("kind", BM.BIN_KINDS)
@pytest.mark.parametrize("bid", BIN_IDS)
def test_bincount(ls, torch_gpu, bid, kind):
    """nbins around the LDS path's limit B = ls.bincount_row_bins(), values inside [0, nbins), at its
    ends, negative and far outside it: one row of 3V + 5 values (several workgroups), 3 rows of V + 1,
    257 rows of 9 and of 100, no values, a view off the 16-byte boundary, all values equal."""
    B, V = ls.bincount_row_bins(), ls.searchsorted_chunk_values()
    nbins = {"0": 0, "1": 1, "255": 255, "256": 256, "B": B, "B+1": B + 1}[bid]
    for rows, nv in ((1, 3 * V + 5), (3, V + 1), (257, 9), (257, 100), (1, 1), (3, 0)):
        x = BM.bincount_words(rows * nv, nbins, 0xB1C + rows, kind).reshape(rows, nv)
        run_bincount(ls, torch_gpu, x[0] if rows == 1 else x, nbins, kind)
    x = BM.bincount_words(2 * V + 7, nbins, 0xB1D, kind)
    run_bincount(ls, torch_gpu, x, nbins, kind, off=1)
    run_bincount(ls, torch_gpu, np.stack([x[:V + 3], x[V + 3:2 * V + 6]]), nbins, kind, off=3)
    for word in (max(nbins - 1, 0), nbins, np.iinfo(SM.word_dtype(kind)).max):
        got = run_bincount(ls, torch_gpu, np.full(2 * V + 9, word, dtype=SM.word_dtype(kind)), nbins, kind, tag="all equal")
        assert int(got.max()) == 2 * V + 9


@pytest.mark.parametrize("kind", ["i32", "u64"])
def test_bincount_more_chunks_than_workgroups(ls, torch_gpu, kind):
    B, V = ls.bincount_row_bins(), ls.searchsorted_chunk_values()
    nv = (4 * cus(torch_gpu) + 3) * V + 5
    for nbins in (1000, B + 1):
        run_bincount(ls, torch_gpu, BM.bincount_words(nv, nbins, 0xB1E, kind), nbins, kind, tag="chunks > grid")


# ---- graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,path", [("f32", "lds"), ("i64", "long"), ("bf16", "long"), ("u32", "lds-store")])
def test_graph_replay(ls, torch_gpu, kind, path):
    """One call captured on a side stream (a single chain: at most a memset, the sample kernel and the
    counting kernel) and replayed on three new (edges, values) sets in the same buffers: the launch
    sequence depends on the host arguments only."""
    torch = torch_gpu
    E, V = EV(ls, kind)
    nedges, rows = (2 * E + 9 if path == "long" else E - 7), 3
    nv = V - 5 if path == "lds-store" else V + 5  # (one workgroup per row, which stores; or two, which add)
    e = SM.esz(kind)
    d_edges = torch.zeros(rows * nedges * e, dtype=torch.uint8, device="cuda")
    d_vals = torch.zeros(rows * nv * e, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(rows * (nedges + 1), dtype=torch.int32, device="cuda")
    need = ls.bucket_counts_workspace_bytes(rows, nedges, kind)
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda") if need else None
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.bucket_counts_device(d_edges, rows, nedges, d_vals, rows, nv, d_out, right=True, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.bucket_counts_device(d_edges, rows, nedges, d_vals, rows, nv, d_out, right=True, key=kind, workspace=ws,
                                stream=torch.cuda.current_stream())
    for j, gen in enumerate(("random", "few", "two")):
        edges, vals, _, right = SM.row_case(gen, rows, nedges, nv, 0x6A0 + j, kind)
        d_edges.copy_(to_dev(torch, edges))
        d_vals.copy_(to_dev(torch, vals))
        d_out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint32).reshape(rows, nedges + 1), BM.counts_of_ranks(right, nedges),
                                      err_msg=f"replay {gen} {kind}")


@pytest.mark.parametrize("which", ["lds", "global"])
def test_bincount_graph_replay(ls, torch_gpu, which):
    torch = torch_gpu
    B, V = ls.bincount_row_bins(), ls.searchsorted_chunk_values()
    nbins, rows, nv = (B if which == "lds" else B + 1), 2, 2 * V + 5
    d_vals = torch.zeros((rows, nv), dtype=torch.int32, device="cuda")
    d_out = torch.zeros((rows, nbins + 1), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ls.bincount_device(d_vals, rows, nv, nbins, d_out, key="i32", stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.bincount_device(d_vals, rows, nv, nbins, d_out, key="i32", stream=torch.cuda.current_stream())
    for j in range(3):
        x = BM.bincount_words(rows * nv, nbins, 0x6B0 + j, "i32").reshape(rows, nv)
        d_vals.copy_(torch.from_numpy(x.view(np.int32).copy()).cuda())
        d_out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint32), BM.bincount_expected(x, nbins, "i32"), err_msg=f"replay {j}")


# ---- ls.bucket_counts / ls.bincount --------------------------------------------------------------------
def torch_keys(torch, kind, shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind in ("i32", "i64"):
        return torch.randint(-1000, 1000, shape, generator=g, dtype=torch.int32 if kind == "i32" else torch.int64).cuda()
    tdt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}[kind]
    return (torch.randn(shape, generator=g, dtype=torch.float32) * 50).to(tdt).cuda()


def by_bucketize(ls, torch, x, edges, right):
    """The route a caller had before: the ranks written out, then torch.bincount (per row: with a row
    offset added)."""
    nb = edges.shape[-1] + 1
    rows = x.shape[0] if x.dim() == 2 else 1
    ranks = (ls.searchsorted(edges, x, right=right) if edges.dim() == 2 else ls.bucketize(x, edges, right=right)).view(rows, -1).long()
    ranks = ranks + torch.arange(rows, device="cuda").view(-1, 1) * nb
    counts = torch.bincount(ranks.flatten(), minlength=rows * nb).int()
    return counts.view(rows, nb) if x.dim() == 2 else counts


@pytest.mark.parametrize("kind", ["i32", "f32", "i64", "f64", "bf16", "f16"])
def test_bucket_counts_against_bucketize_and_torch_bincount(ls, torch_gpu, kind):
    torch = torch_gpu
    E, V = EV(ls, kind)
    for nedges in (255, E + 3):
        edges = torch_keys(torch, kind, (3, nedges), 0x70 + nedges).sort(dim=-1).values.contiguous()
        x = torch.cat([torch_keys(torch, kind, (3, V + 5), 0x71), edges[:, :100]], dim=-1).contiguous()
        for right in (False, True):
            got = ls.bucket_counts(x, edges, right=right)
            assert got.dtype == torch.int32 and got.shape == (3, nedges + 1)
            assert torch.equal(got, by_bucketize(ls, torch, x, edges, right)), (kind, nedges, right, "per-row edges")
            got = ls.bucket_counts(x, edges[1].contiguous(), right=right)
            assert got.shape == (3, nedges + 1) and torch.equal(got, by_bucketize(ls, torch, x, edges[1].contiguous(), right))
            got = ls.bucket_counts(x[2].contiguous(), edges[0].contiguous(), right=right)
            assert got.shape == (nedges + 1,) and torch.equal(got, by_bucketize(ls, torch, x[2].contiguous(), edges[0].contiguous(), right))
            assert int(got.sum()) == x.shape[1]
    # empty ends
    edges = torch_keys(torch, kind, (50,), 5).sort().values
    x = torch_keys(torch, kind, (4, 30), 6)
    assert torch.equal(ls.bucket_counts(x[:, :0].contiguous(), edges), torch.zeros((4, 51), dtype=torch.int32, device="cuda"))
    assert torch.equal(ls.bucket_counts(x, edges[:0]), torch.full((4, 1), 30, dtype=torch.int32, device="cuda"))
    assert ls.bucket_counts(x[:0], edges).shape == (0, 51)
    assert torch.equal(ls.bucket_counts(x[0, :0].contiguous(), edges), torch.zeros(51, dtype=torch.int32, device="cuda"))


def test_bucket_counts_shape_errors(ls, torch_gpu):
    torch = torch_gpu
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="do not match"):
        ls.bucket_counts(z(3, 10), z(2, 5))
    with pytest.raises(ValueError, match="do not match"):
        ls.bucket_counts(z(10), z(1, 5))
    with pytest.raises(ValueError, match="1-D or 2-D"):
        ls.bucket_counts(z(2, 3, 4), z(5))
    with pytest.raises(ValueError, match="1-D or 2-D"):
        ls.bincount(z(2, 3, 4), 5)
    with pytest.raises(ValueError, match="nbins"):
        ls.bincount(z(5), -1)


@pytest.mark.parametrize("kind", ["i32", "i64"])
def test_bincount_against_torch_bincount(ls, torch_gpu, kind):
    torch = torch_gpu
    B, V = ls.bincount_row_bins(), ls.searchsorted_chunk_values()
    tdt = torch.int32 if kind == "i32" else torch.int64
    g = torch.Generator(device="cpu").manual_seed(0xB1)
    for nbins in (1000, B + 1):
        x = torch.randint(0, nbins, (3, 2 * V + 5), generator=g, dtype=tdt).cuda()
        got = ls.bincount(x, nbins)
        assert got.dtype == torch.int32 and got.shape == (3, nbins + 1)
        for r in range(3):
            assert torch.equal(got[r, :nbins], torch.bincount(x[r], minlength=nbins).int()) and int(got[r, nbins]) == 0
        got1 = ls.bincount(x[1].contiguous(), nbins)
        assert got1.shape == (nbins + 1,) and torch.equal(got1, got[1])
        # what torch.bincount refuses (a negative value) or would grow its result for is counted in the last word
        y = x.clone()
        y[:, ::7] = -3
        y[:, 1::7] = nbins + 5
        got = ls.bincount(y, nbins)
        for r in range(3):
            inside = y[r][(y[r] >= 0) & (y[r] < nbins)]
            assert torch.equal(got[r, :nbins], torch.bincount(inside, minlength=nbins).int())
            assert int(got[r, nbins]) == y.shape[1] - inside.numel()
    assert torch.equal(ls.bincount(x[:, :0].contiguous(), 7), torch.zeros((3, 8), dtype=torch.int32, device="cuda"))
    assert ls.bincount(x[:0], 7).shape == (0, 8)
