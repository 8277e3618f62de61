"""GPU tests of labsort_unique_device / ls.unique_device / ls.unique against the numpy model
(tests/unique_model.py): every requested output, m and the sentinel past m compared bit for bit, the
input unchanged.  C = ls.unique_chunk_keys() is the chunk of the run-edge passes; the workspace of
every call is filled with garbage first and sized for exactly the outputs that are passed."""
import functools

import numpy as np
import pytest

import unique_model as U

pytestmark = pytest.mark.gpu

S32 = np.uint32(U.SENTINEL32)
S64 = np.uint64((U.SENTINEL32 << 32) | U.SENTINEL32)
COUNTS, FIRST, INVERSE = 1, 2, 4
ALL = COUNTS | FIRST | INVERSE


def signed(a):
    return a.view(np.int64 if a.dtype == np.uint64 else np.int32)


def run(ls, torch, x, kind, consecutive=False, outputs=ALL, exp=None, tag=""):
    """One unique_device call on the words x, checked against the model."""
    x = np.ascontiguousarray(x, dtype=U.word_dtype(kind))
    n = x.size
    values, counts, first, inverse, m = exp if exp is not None else U.expected(x, kind, consecutive)
    sent = S64 if x.dtype == np.uint64 else S32
    dev = lambda a: torch.from_numpy(signed(a).copy()).cuda()  # noqa: E731
    words = lambda on: dev(np.full(n, S32, dtype=np.uint32)) if on else None  # noqa: E731
    d_keys = dev(x)
    d_uniq = dev(np.full(n, sent, dtype=x.dtype))
    d_num = dev(np.full(1, S32, dtype=np.uint32))
    d_counts, d_first, d_inverse = words(outputs & COUNTS), words(outputs & FIRST), words(outputs & INVERSE)
    pos = bool(outputs & (FIRST | INVERSE))
    ws = torch.full((ls.unique_workspace_bytes(n, kind, consecutive, pos),), 0xCD, dtype=torch.uint8, device="cuda")
    ls.unique_device(d_keys, n, d_uniq, d_num, d_counts, d_first, d_inverse, key=kind, consecutive=consecutive, workspace=ws)
    ls.unique_workspace_status(ws, n, kind, consecutive)  # (synchronises)
    check(x, d_keys, d_uniq, d_num, d_counts, d_first, d_inverse, (values, counts, first, inverse, m),
          f"{tag} {kind} n={n} consecutive={consecutive} outputs={outputs}")


def check(x, d_keys, d_uniq, d_num, d_counts, d_first, d_inverse, exp, msg):
    values, counts, first, inverse, m = exp
    host = lambda t: t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)  # noqa: E731
    sent = S64 if x.dtype == np.uint64 else S32
    assert int(host(d_num)[0]) == m, f"m: {msg}"
    got = host(d_uniq)
    np.testing.assert_array_equal(got[:m], values, err_msg=f"values: {msg}")
    assert np.all(got[m:] == sent), f"values past m written: {msg}"
    for name, t, want in (("counts", d_counts, counts), ("first", d_first, first)):
        if t is not None:
            got = host(t)
            np.testing.assert_array_equal(got[:m], want, err_msg=f"{name}: {msg}")
            assert np.all(got[m:] == S32), f"{name} past m written: {msg}"
    if d_inverse is not None:
        np.testing.assert_array_equal(host(d_inverse), inverse, err_msg=f"inverse: {msg}")
    np.testing.assert_array_equal(host(d_keys), x, err_msg=f"the input was written: {msg}")


def chunk(ls):
    return ls.unique_chunk_keys()


# ---- sizes -----------------------------------------------------------------------------------------
SIZE_IDS = ["1", "2", "63", "64", "65", "C-1", "C", "C+1", "3C+5", "2^18+3", "65C+7", "1025C+9"]


def size_of(C, sid):
    return U.sizes(C)[SIZE_IDS.index(sid)] if sid in SIZE_IDS[:10] else 65 * C + 7 if sid == "65C+7" else 1025 * C + 9


@pytest.mark.parametrize("kind", ["u32", "i64"])
@pytest.mark.parametrize("sid", SIZE_IDS)
def test_sizes(ls, torch_gpu, sid, kind):
    """One wave's worth and its neighbours, a chunk's edges, several chunks, past the pair sort's switch
    to its radix path (2^18 + 3), past CP_SCAN_SERIAL chunks (the block scan) and past 1024 chunks (its
    second step); both modes, every output.  Sorted: 1000 values (at 65C + 7: full-width words, m = n or
    nearly); consecutive: ascending runs of 1 to 3000 elements."""
    n = size_of(chunk(ls), sid)
    for consecutive in (False, True):
        gen = "sorted_runs" if consecutive else "uniform" if sid == "65C+7" else "mod1000"
        x, exp = U.case(gen, n, 0x0051 + n, kind, consecutive)
        run(ls, torch_gpu, x, kind, consecutive, ALL, exp, tag=gen)


# ---- run shapes at 3C + 5 ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_input(name, C):
    n = 3 * C + 5
    i = np.arange(n, dtype=np.int64)
    if name == "all_equal":
        v = np.full(n, 42)
    elif name == "all_distinct":
        v = np.random.default_rng(0x5A).permutation(n) * 3 - n
    elif name == "three_chunks_one_run":
        v = np.concatenate([np.full(3 * C, 7), [8, 9, 9, 10, 11]])
    elif name == "edges_on_chunk_ends":
        v = (i // C) * 1000 + (i % C) // 37  # a run ends on every chunk's last element, the next starts on the first
        assert v[C - 1] != v[C] and v[C - 2] == v[C - 1] and v[C] == v[C + 1]
    elif name == "singles_at_both_ends":
        v = np.concatenate([[0], np.full(n - 2, 5), [9]])
    elif name == "i_div_3":
        v = i // 3
    elif name == "i_mod_7":
        v = i % 7
    v = np.asarray(v, dtype=np.int64)
    v.setflags(write=False)
    return v


SHAPES = ["all_equal", "all_distinct", "three_chunks_one_run", "edges_on_chunk_ends", "singles_at_both_ends", "i_div_3",
          "i_mod_7"]


@pytest.mark.parametrize("kind", ["i32", "u64"])
@pytest.mark.parametrize("name", SHAPES)
def test_run_shapes(ls, torch_gpu, name, kind):
    C = chunk(ls)
    v = shape_input(name, C)
    x = U.from_ints(v - v.min() if kind == "u64" else v, kind)
    for consecutive in (False, True):
        exp = U.expected(x, kind, consecutive)
        if name == "all_equal":
            assert exp[4] == 1
        if name == "all_distinct" or (name == "i_mod_7" and consecutive):
            assert exp[4] == x.size
        if name == "i_mod_7" and not consecutive:
            assert exp[4] == 7
        run(ls, torch_gpu, x, kind, consecutive, ALL, exp, tag=name)


# ---- every combination of the optional outputs -----------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "i64"])
@pytest.mark.parametrize("outputs", range(8))
def test_output_combinations(ls, torch_gpu, outputs, kind):
    """C + 1 keys; run() sizes the workspace with positions=False for the combinations without first
    and inverse, which therefore must not touch the positions' part."""
    n = chunk(ls) + 1
    for consecutive in (False, True):
        x, exp = U.case("mod1000", n, 0x0C0B, kind, consecutive)
        if not outputs & (FIRST | INVERSE):
            assert ls.unique_workspace_bytes(n, kind, consecutive, False) <= ls.unique_workspace_bytes(n, kind, consecutive, True)
        run(ls, torch_gpu, x, kind, consecutive, outputs, exp)


# ---- key types -----------------------------------------------------------------------------------------
def planted(pool, n, seed, dtype):
    rng = np.random.default_rng(seed)
    pool = np.array(pool, dtype=dtype)
    return np.concatenate([pool, pool[rng.integers(0, pool.size, size=n - pool.size)]])


F32_POOL = [0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000, 0x3F800000, 0xBF800000,
            0x7FC00000, 0xFFC00001, 0x7F800001, 0xFF812345, 0x7FFFFFFF]
F64_POOL = [0xFFF0000000000000, 1 << 63, 0, 1, (1 << 63) | 1, 0x000FFFFFFFFFFFFF, 0x7FF0000000000000, 0x3FF0000000000000,
            0xBFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF4000000012345,
            0x7FFFFFFFFFFFFFFF]
HALVES = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
WIDE_POOL = [(a << 32) | b for a in HALVES for b in HALVES]  # keys that differ in one 32-bit half only


@pytest.mark.parametrize("consecutive", [False, True])
@pytest.mark.parametrize("kind,pool", [("i32", [0x80000000, 0xFFFFFFFF, 0, 1, 0x7FFFFFFF, 0xFFFFFF00, 0x80000001]),
                                       ("f32", F32_POOL), ("f64", F64_POOL), ("u64", WIDE_POOL), ("i64", WIDE_POOL),
                                       ("f64", WIDE_POOL), ("u64", [(1 << 63) + 5, (1 << 63) - 1, (1 << 64) - 1, 1 << 63, 7])],
                         ids=["i32-negatives", "f32-specials", "f64-specials", "u64-halves", "i64-halves", "f64-halves",
                              "u64-above-2^63"])
def test_key_types(ls, torch_gpu, kind, pool, consecutive):
    """Negative int32 keys; floats with -inf, both zeros, subnormals and NaNs of both signs and several
    payloads (one entry, 0x7FFF..); 64-bit keys that differ only in the high or only in the low word,
    which a 32-bit compare would merge; uint64 keys above 2^63."""
    n = chunk(ls) + 77
    x = planted(pool, n, 0x7E57 + len(pool), U.word_dtype(kind))
    exp = U.expected(x, kind, consecutive)
    if not consecutive:
        assert exp[4] == np.unique(U.image(np.array(pool, dtype=x.dtype), kind)).size
    run(ls, torch_gpu, x, kind, consecutive, ALL, exp)


def test_consecutive_keeps_separate_runs(ls, torch_gpu):
    """[3, 3, 1, 3, 3, 3, 1, 1] tiled past two chunks: nothing is sorted, equal keys in separate runs
    stay separate."""
    reps = 2 * chunk(ls) // 8 + 3
    v = np.tile(np.array([3, 3, 1, 3, 3, 3, 1, 1], dtype=np.int64), reps)
    for kind in ("u32", "i64"):
        x = U.from_ints(v, kind)
        exp = U.expected(x, kind, True)
        assert exp[4] == 4 * reps
        run(ls, torch_gpu, x, kind, True, ALL, exp)
        run(ls, torch_gpu, x, kind, False, ALL)  # and sorted by the call: two values


def test_nothing_to_do(ls, torch_gpu):
    """n == 0: *d_num_out = 0 and nothing else, d_keys may be NULL and the workspace is not looked at."""
    torch = torch_gpu
    for kind in ("u32", "f64"):
        uniq = torch.full((4,), 77, dtype=torch.int64, device="cuda")
        num = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        st = ls.lib.labsort_unique_device(None, 0, ls.KEY[kind], 0, uniq.data_ptr(), None, None, None, num.data_ptr(), None, 0,
                                          torch.cuda.current_stream().cuda_stream)
        assert st == ls.OK
        torch.cuda.synchronize()
        assert int(num.item()) == 0 and bool((uniq == 77).all())
        ls.unique_workspace_status(uniq, 0, kind)
    assert ls.unique(torch.zeros(0, dtype=torch.int32, device="cuda")).numel() == 0


# ---- seeded sweep --------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(40))
def test_sweep_seed_7171(ls, torch_gpu, i):
    c = list(U.sweep_cases(0x7171, chunk(ls)))[i]
    x, exp = U.case(c["gen"], c["n"], c["seed"], c["kind"], c["consecutive"])
    run(ls, torch_gpu, x, c["kind"], c["consecutive"], c["outputs"], exp, tag=c["tag"])


# ---- graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["i64", "i32"])
def test_graph_replay(ls, torch_gpu, kind):
    """One unique_device call captured on a side stream and replayed on three key sets of the same n with
    different m: the launch sequence depends on the host arguments only and m stays on the device."""
    torch = torch_gpu
    n = 3 * chunk(ls) + 5
    dt = torch.int64 if kind == "i64" else torch.int32
    d_keys = torch.zeros(n, dtype=dt, device="cuda")
    d_uniq = torch.zeros(n, dtype=dt, device="cuda")
    d_num = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_counts, d_first, d_inverse = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    ws = torch.full((ls.unique_workspace_bytes(n, kind),), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_keys, n, d_uniq, d_num, d_counts, d_first, d_inverse)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.unique_device(*args, key=kind, workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.unique_device(*args, key=kind, workspace=ws, stream=torch.cuda.current_stream())
    seen = set()
    for gen in ("mod17", "uniform", "mod1000"):
        x, exp = U.case(gen, n, 0x6A0 + len(gen), kind, False)
        seen.add(exp[4])
        d_keys.copy_(torch.from_numpy(signed(x).copy()))
        for t in (d_uniq, d_counts, d_first, d_inverse, d_num):
            t.copy_(torch.from_numpy(signed(np.full(t.numel(), S64 if t.element_size() == 8 else S32))))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.unique_workspace_status(ws, n, kind)
        check(x, d_keys, d_uniq, d_num, d_counts, d_first, d_inverse, exp, f"replay {gen} {kind}")
    assert len(seen) == 3


# ---- ls.unique -----------------------------------------------------------------------------------------
def test_unique_against_torch(ls, torch_gpu):
    """int64: the two contracts agree on integers (values sorted, inverse, counts); index is the first
    occurrence; consecutive mode against torch.unique_consecutive."""
    torch = torch_gpu
    gen = torch.Generator(device="cpu").manual_seed(0x70C4)
    x = torch.randint(-500, 500, (3 * chunk(ls) + 5,), generator=gen, dtype=torch.int64).cuda()
    values, inverse, counts, index = ls.unique(x, return_inverse=True, return_counts=True, return_index=True)
    tv, ti, tc = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
    assert values.dtype == torch.int64 and inverse.dtype == counts.dtype == index.dtype == torch.int32
    assert torch.equal(values, tv) and torch.equal(inverse.long(), ti) and torch.equal(counts.long(), tc)
    assert torch.equal(x[index.long()], values) and torch.equal(values[inverse.long()], x)
    first = torch.full_like(tv, x.numel()).scatter_reduce(0, ti, torch.arange(x.numel(), device="cuda"), "amin")
    assert torch.equal(index.long(), first)
    only = ls.unique(x)
    assert isinstance(only, torch.Tensor) and torch.equal(only, tv)
    v2, c2 = ls.unique(x, return_counts=True)
    assert torch.equal(v2, tv) and torch.equal(c2.long(), tc)
    y = torch.sort(x).values.remainder(7)
    cv, ci, cc = ls.unique(y, return_inverse=True, return_counts=True, consecutive=True)
    ev, ei, ec = torch.unique_consecutive(y, return_inverse=True, return_counts=True)
    assert torch.equal(cv, ev) and torch.equal(ci.long(), ei) and torch.equal(cc.long(), ec)
    f = torch.tensor([0.0, -0.0, float("nan"), 1.5, float("nan"), -0.0], device="cuda")
    fv, fc = ls.unique(f, return_counts=True)
    assert fc.tolist() == [2, 1, 1, 2] and fv[:3].tolist() == [-0.0, 0.0, 1.5] and bool(torch.isnan(fv[3]))
    assert bool(torch.signbit(fv[0])) and not bool(torch.signbit(fv[1]))
