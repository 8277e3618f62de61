"""GPU tests of labsort_unique_device / ls.unique_device / ls.unique against the numpy model
(tests/unique_model.py): every requested output, m and the sentinel past m compared bit for bit, the
input unchanged.  C = ls.unique_chunk_keys() is the chunk of the run-edge passes.

Guards.  run() places the keys, every output and the one word of m inside a storage of its own with
GUARD_BYTES (512: 64 elements of the widest type) of the byte 0x3C in front and behind, which is
neither the outputs' pre-fill 0xA5 nor the workspace's 0xCD / 0xFF, and check() asserts that every
guard byte is unchanged, naming the buffer and the side.  The workspace is a view 256 bytes into a
storage of 512 bytes more than is asked for, with the same guard byte on both sides; unless a case
passes its own it is sized for exactly the outputs that are passed and filled with 0xCD.

Offsets.  in_off, uniq_off, counts_off, first_off and inv_off are counted in elements from a 256-byte
aligned address, so a buffer's address is off * element size mod 256; Guarded asserts that residue
mod 16, and the cases that rely on an unaligned (or aligned) pointer assert which one they have.

Workspace alignment.  Every workspace here starts on a 256-byte boundary, as the allocator's do: no
entry of the library but searchsorted defines a smaller one, and none is tested."""
import functools

import numpy as np
import pytest

import unique_model as U
import whole_sort_model as W

pytestmark = pytest.mark.gpu

S32 = np.uint32(U.SENTINEL32)
S64 = np.uint64((U.SENTINEL32 << 32) | U.SENTINEL32)
COUNTS, FIRST, INVERSE = 1, 2, 4
ALL = COUNTS | FIRST | INVERSE
GUARD_BYTE, GUARD_BYTES = 0x3C, 512
SENT_BYTE = U.SENTINEL32 & 0xFF
assert U.SENTINEL32 == SENT_BYTE * 0x01010101 and GUARD_BYTE not in (SENT_BYTE, 0xCD, 0xFF)


def signed(a):
    return a.view(np.int64 if a.dtype == np.uint64 else np.int32)


class Guarded:
    """n elements of esize bytes, `off` elements behind a 256-byte aligned address, with `lead` guard
    bytes in front of that address and at least as many behind the last element.  view: the elements
    (int32, int64, or uint8 for esize 1), filled with the byte `fill`."""

    def __init__(self, torch, name, n, esize, off=0, fill=SENT_BYTE, lead=GUARD_BYTES):
        assert lead % 256 == 0 and lead >= 64 * esize
        self.name, self.lo = name, lead + off * esize
        self.hi = self.lo + n * esize
        self.store = torch.full((self.hi + lead,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        assert self.store.data_ptr() % 256 == 0
        body = self.store[self.lo:self.hi]
        body.fill_(fill)
        self.view = body if esize == 1 else body.view(torch.int64 if esize == 8 else torch.int32)
        assert self.view.numel() == n and self.view.data_ptr() % 16 == (off * esize) % 16

    def check(self, msg):
        for side, part in (("in front of", self.store[:self.lo]), ("behind", self.store[self.hi:])):
            assert bool((part == GUARD_BYTE).all()), f"the guard {side} {self.name} was written: {msg}"


def workspace(torch, nbytes, fill=0xCD):
    """A guarded workspace of nbytes on a 256-byte boundary, 256 bytes into its storage."""
    g = Guarded(torch, "the workspace", nbytes, 1, fill=fill, lead=256)
    assert g.view.data_ptr() % 256 == 0
    return g


def run(ls, torch, x, kind, consecutive=False, outputs=ALL, exp=None, tag="", in_off=0, uniq_off=0, counts_off=0,
        first_off=0, inv_off=0, ws=None, ws_positions=False):
    """One unique_device call on the words x, checked against the model.  *_off: elements between a
    256-byte aligned address and the buffer.  ws: a Guarded workspace (workspace()) that is used as it
    is and not cleared; without one, one of exactly the size asked for, with positions when the call
    passes first or inverse or when ws_positions is set."""
    x = np.ascontiguousarray(x, dtype=U.word_dtype(kind))
    n, esize = x.size, x.dtype.itemsize
    exp = exp if exp is not None else U.expected(x, kind, consecutive)
    keys = Guarded(torch, "the keys", n, esize, in_off)
    keys.view.copy_(torch.from_numpy(signed(x).copy()))
    uniq = Guarded(torch, "unique_out", n, esize, uniq_off)
    num = Guarded(torch, "num_out", 1, 4)
    words = lambda on, name, off: Guarded(torch, name, n, 4, off) if on else None  # noqa: E731
    counts = words(outputs & COUNTS, "counts_out", counts_off)
    first = words(outputs & FIRST, "first_out", first_off)
    inverse = words(outputs & INVERSE, "inverse_out", inv_off)
    if ws is None:
        pos = bool(outputs & (FIRST | INVERSE)) or ws_positions
        ws = workspace(torch, ls.unique_workspace_bytes(n, kind, consecutive, pos))
    view = lambda g: None if g is None else g.view  # noqa: E731
    msg = f"{tag} {kind} n={n} consecutive={consecutive} outputs={outputs}"
    ls.unique_device(keys.view, n, uniq.view, num.view, view(counts), view(first), view(inverse), key=kind,
                     consecutive=consecutive, workspace=ws.view)
    try:
        ls.unique_workspace_status(ws.view, n, kind, consecutive)  # (synchronises)
    except ls.LabsortError as e:
        raise AssertionError(f"unique_workspace_status: {e}: {msg}") from e
    check(x, keys.view, uniq.view, num.view, view(counts), view(first), view(inverse), exp, msg,
          guards=[g for g in (keys, uniq, num, counts, first, inverse, ws) if g is not None])


def check(x, d_keys, d_uniq, d_num, d_counts, d_first, d_inverse, exp, msg, guards=()):
    values, counts, first, inverse, m = exp
    for g in guards:
        g.check(msg)
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


# ---- unaligned views -----------------------------------------------------------------------------------
ODD = dict(uniq_off=1, counts_off=3, first_off=5, inv_off=7)  # every output at an odd offset of its own
EVEN = dict(uniq_off=0, counts_off=0, first_off=0, inv_off=0)
# (keys' offset in elements, the outputs' offsets): every unaligned residue of the keys with unaligned
# outputs, then aligned keys with unaligned outputs and unaligned keys with aligned outputs
VIEWS4 = [(1, ODD), (2, ODD), (3, ODD), (0, ODD), (1, EVEN)]
VIEWS8 = [(1, ODD), (0, ODD), (1, EVEN)]
VIEW_CASES = [(k, i) for k in ("u32", "f32") for i in range(len(VIEWS4))] + \
             [(k, i) for k in ("i64", "f64") for i in range(len(VIEWS8))]


@functools.lru_cache(maxsize=None)
def runs_case(div, n, kind):
    """i // div as keys of the kind, with the consecutive mode's expectation (read-only)."""
    x = U.from_ints(np.arange(n, dtype=np.int64) // div, kind)
    exp = U.expected(x, kind, True)
    U.freeze(x, *exp)
    return x, exp


@pytest.mark.parametrize("kind,view", VIEW_CASES, ids=[f"{k}-{i}" for k, i in VIEW_CASES])
def test_unaligned_views(ls, torch_gpu, kind, view):
    """Keys 4, 8 or 12 bytes (8-byte kinds: 8 bytes) past a 16-byte boundary and every output at an odd
    element offset of its own: uq_load_heads reads every group of every chunk element by element in
    consecutive mode, k_uq_iota_copy takes its element-wise branch in the pair sort's, the keys-only
    sort and sort64 read an unaligned input.  n = 2C + 3 (two full chunks and one of three elements:
    full groups, the partial group and lane 0's read across a chunk's end) and 65; ALL (pair sort),
    COUNTS (keys sort) and no optional output.  Consecutive mode on i // 3 and i // 5, whose heads fall
    on different lanes from group to group, so an element loaded from the wrong place changes m;
    sorted mode on mod1000 and full-width words."""
    wide = kind in U.KINDS64
    in_off, outs = (VIEWS8 if wide else VIEWS4)[view]
    esize = 8 if wide else 4
    # the residues mod 16 that this configuration is about (Guarded asserts each pointer's against its offset)
    residues = {"keys": in_off * esize % 16, "unique_out": outs["uniq_off"] * esize % 16,
                **{name: outs[name] * 4 % 16 for name in ("counts_off", "first_off", "inv_off")}}
    assert (residues["keys"] != 0) == (in_off != 0) and residues["keys"] == (in_off * esize if in_off else 0)
    assert all(r != 0 for name, r in residues.items() if name != "keys") if outs is ODD else outs is EVEN
    assert len({outs[name] for name in outs}) == (4 if outs is ODD else 1)
    assert in_off or outs is ODD  # (something is unaligned in every configuration)
    C = chunk(ls)
    for n in (2 * C + 3, 65):
        for outputs in (ALL, COUNTS, 0):
            for div in (3, 5):
                x, exp = runs_case(div, n, kind)
                assert exp[4] == (n + div - 1) // div
                run(ls, torch_gpu, x, kind, True, outputs, exp, tag=f"i//{div} in_off={in_off}", in_off=in_off, **outs)
            for gen in ("mod1000", "uniform"):
                x, exp = U.case(gen, n, 0x0A11 + n, kind, False)
                run(ls, torch_gpu, x, kind, False, outputs, exp, tag=f"{gen} in_off={in_off}", in_off=in_off, **outs)


# ---- the workspace contract ----------------------------------------------------------------------------
def reuse_sequence(C):
    """(n, kind, consecutive, outputs, generator): sizes, key widths, modes and output sets in turn.
    Call 1 is a keys-only sort of one tile on the untouched garbage: it has no status word, so its
    status must not read one.  Calls 2-4: a pair sort (radix), a consecutive call, a keys-only sort of
    a smaller n.  Calls 5-6: a 64-bit call, then a 4-byte one.  Call 11: a keys-only sort of one tile
    behind a 64-bit call's use of the same bytes."""
    big = (1 << 18) + 3
    return [(3 * C + 5, "u32", False, COUNTS, "mod1000"),
            (big, "u32", False, ALL, "uniform"),
            (3 * C + 5, "i32", True, ALL, "sorted_runs"),
            (C + 1, "u32", False, COUNTS, "mod1000"),
            (big, "i64", False, ALL, "mod1000"),
            (65, "f32", False, FIRST, "mod17"),
            (big, "f32", False, 0, "uniform"),
            (3 * C + 5, "f64", True, COUNTS | INVERSE, "sorted_runs"),
            (3 * C + 5, "u32", False, ALL, "mod1000"),
            (C + 1, "u64", False, COUNTS, "uniform"),
            (3 * C + 5, "i32", False, COUNTS, "mod17"),
            (65, "u64", True, ALL, "mod17"),
            (big, "i32", False, COUNTS | INVERSE, "mod1000"),
            (65, "u32", False, 0, "uniform")]


def test_workspace_reuse(ls, torch_gpu):
    """One workspace, sized with positions for the largest call of the sequence, filled with 0xFF once
    and never cleared, serves fourteen calls of changing n, key width, mode and output set: every
    output is exact, no guard is touched and unique_workspace_status with the call's own (n, kind,
    consecutive) is OK after each (run() raises otherwise), although header word UQ_HDR_SORT and the
    inner sort's status word are whatever the calls before left there."""
    seq = reuse_sequence(chunk(ls))
    assert len(seq) >= 12 and {c[0] for c in seq} == {65, chunk(ls) + 1, 3 * chunk(ls) + 5, (1 << 18) + 3}
    pair = lambda c: c[1] in U.KINDS32 and not c[2] and bool(c[3] & (FIRST | INVERSE))  # noqa: E731
    keys = lambda c: c[1] in U.KINDS32 and not c[2] and not c[3] & (FIRST | INVERSE)  # noqa: E731
    assert any(pair(a) and b[2] and keys(c) and c[0] < a[0] for a, b, c in zip(seq, seq[1:], seq[2:]))
    assert any(a[1] in U.KINDS64 and b[1] in U.KINDS32 for a, b in zip(seq, seq[1:]))
    assert keys(seq[0]) and ls.pair_tile_keys() < seq[0][0] <= ls.tile_keys()
    ws = workspace(torch_gpu, max(ls.unique_workspace_bytes(n, kind, cons, True) for n, kind, cons, _, _ in seq), fill=0xFF)
    for i, (n, kind, cons, outputs, gen) in enumerate(seq):
        assert ws.view.numel() >= ls.unique_workspace_bytes(n, kind, cons, bool(outputs & (FIRST | INVERSE)))
        x, exp = U.case(gen, n, 0x2E05 + i, kind, cons)
        run(ls, torch_gpu, x, kind, cons, outputs, exp, tag=f"reuse call {i + 1} {gen}", ws=ws)


@pytest.mark.parametrize("kind", ["u32", "f32", "i64"])
def test_oversized_workspace(ls, torch_gpu, kind):
    """The output sets without first and inverse on a workspace sized with positions, and every kind
    of call on one sized for 2 n keys: the layout is the call's own, whatever the size.  n = 3C + 5
    (one tile of the keys-only sort, a merge of pairs) and 2^16 + 1 (the gathered radix without
    positions, whose layout shares nothing with the merge sort's)."""
    for n in (3 * chunk(ls) + 5, ls.GS_MIN_N + 1):
        for consecutive in (False, True):
            x, exp = U.case("mod1000", n, 0x0B16, kind, consecutive)
            for outputs in (0, COUNTS):
                with_pos, without = (ls.unique_workspace_bytes(n, kind, consecutive, p) for p in (True, False))
                assert with_pos >= without
                run(ls, torch_gpu, x, kind, consecutive, outputs, exp, tag="sized with positions", ws_positions=True)
            for outputs in (0, COUNTS, ALL):
                pos = bool(outputs & (FIRST | INVERSE))
                twice = ls.unique_workspace_bytes(2 * n, kind, consecutive, pos)
                assert twice >= ls.unique_workspace_bytes(n, kind, consecutive, pos)
                run(ls, torch_gpu, x, kind, consecutive, outputs, exp, tag="sized for 2n", ws=workspace(torch_gpu, twice))


# ---- every inner-sort route ----------------------------------------------------------------------------
ROUTE_CLASSES = ("tile_sort", "merge", "merge4", "gsweep", "gcopy", "histogram", "onesweep")


def route_of(ls, n, pairs):
    """The sort that LABSORT_ALGO_AUTO runs for n 4-byte keys (api.hip: resolve_algo, small_path and
    use_gather for the keys-only entry, resolve_pairs_algo and the one-tile test for key/value)."""
    if pairs:
        return "tile" if n <= ls.pair_tile_keys() else "merge" if n <= W.constants()["AUTO_PAIRS_MERGE_MAX_KEYS"] else "onesweep"
    return "tile" if n <= ls.tile_keys() else "merge" if n <= ls.GS_MIN_N else ls.radix_impl(n)


def run_routed(ls, torch, x, kind, outputs, exp, tag):
    """run() with the timing hooks on; the launches that the inner sort's classes counted must be the
    route's: one tile sort alone; one tile sort and merge passes; gathered passes and their copy; one
    histogram and four onesweep passes."""
    route = route_of(ls, x.size, bool(outputs & (FIRST | INVERSE)))
    ls.timing_enable(True)
    try:
        run(ls, torch, x, kind, False, outputs, exp, tag=f"{tag} route={route}")
        got = {c: ls.timing_read(c)[1] for c in ROUTE_CLASSES}
    finally:
        ls.timing_enable(False)
    merges, gathered = got["merge"] + got["merge4"], got["gsweep"]
    want = {"tile": got["tile_sort"] == 1 and merges == 0 and gathered == 0 and got["onesweep"] == 0,
            "merge": got["tile_sort"] == 1 and merges >= 1 and gathered == 0 and got["onesweep"] == 0,
            "gather": got["tile_sort"] == 0 and merges == 0 and gathered >= 1 and got["gcopy"] == 1 and got["onesweep"] == 0,
            "onesweep": got["tile_sort"] == 0 and merges == 0 and gathered == 0 and got["histogram"] == 1 and got["onesweep"] == 4}
    assert want[route], f"{tag} n={x.size} outputs={outputs}: route {route} expected, launches {got}"
    return route


ROUTE_IDS = [i for i, _ in U.route_sizes(1, 1, 1, 1)]


@pytest.mark.parametrize("outputs", [ALL, COUNTS], ids=["pairs", "keys"])
@pytest.mark.parametrize("sid", ROUTE_IDS)
@pytest.mark.parametrize("kind", U.KINDS32)
def test_inner_sort_routes(ls, torch_gpu, kind, sid, outputs):
    """The sizes at which the inner sort of 4-byte keys changes algorithm, one below, at and one above,
    with every output (labsort_sort_pairs_device) and with counts only (labsort_sort_device).  By
    api.hip, with LABSORT_ALGO_AUTO:
      keys   n <= tile_keys() (32768): one tile sort, no workspace; n <= 2^16: tile sort and merge
             passes; 2^16 < n < 2^25: the gathered radix; from 2^25: histogram, plan and onesweep passes;
      pairs  n <= pair_tile_keys() (16384): one key/value tile sort; n <= 2^18: tile sort and merge
             passes; above: histogram, plan and onesweep passes with payloads (no gathered radix).
    So 2^18 is no edge of the keys-only route and tile_keys() and 2^16 are none of the pairs'; they are
    edges of the workspace layout all the same (uq_inner_bytes).  The timing hooks tell the routes
    apart by launch counts (run_routed); they do not tell a keys-only from a key/value launch of the
    same class.  Full-width words (m = n or nearly) and 1000 values at every size."""
    sizes = dict(U.route_sizes(ls.pair_tile_keys(), ls.tile_keys(), ls.GS_MIN_N, W.constants()["AUTO_PAIRS_MERGE_MAX_KEYS"]))
    assert sizes["pair_tile"] == ls.pair_tile_keys() < sizes["tile"] == ls.tile_keys() < sizes["2^16"] == 1 << 16
    assert sizes["2^18"] == 1 << 18 and list(sizes) == ROUTE_IDS
    n = sizes[sid]
    routes = set()
    for gen in ("uniform", "mod1000"):
        x, exp = U.case(gen, n, 0x4007 + n, kind, False)
        assert exp[4] <= 1000 if gen == "mod1000" else exp[4] > n - n // 64 - 8  # (f32: the NaNs are one value)
        routes.add(run_routed(ls, torch_gpu, x, kind, outputs, exp, gen))
    pairs = outputs == ALL
    edge, d = (sid[:-2], int(sid[-2:])) if sid[-2] in "+-" else (sid, 0)
    low, high = {("pair_tile", True): ("tile", "merge"), ("tile", True): ("merge", "merge"), ("2^16", True): ("merge", "merge"),
                 ("2^18", True): ("merge", "onesweep"), ("pair_tile", False): ("tile", "tile"), ("tile", False): ("tile", "merge"),
                 ("2^16", False): ("merge", "gather"), ("2^18", False): ("gather", "gather")}[(edge, pairs)]
    assert routes == {high if d > 0 else low}


LARGE = [((1 << 25) - 1, ALL), (1 << 25, ALL), ((1 << 25) - 1, COUNTS), (1 << 25, COUNTS)]


@pytest.mark.parametrize("V", [1000, (1 << 20) + 7])
@pytest.mark.parametrize("n,outputs", LARGE, ids=["2^25-1-pairs", "2^25-pairs", "2^25-1-keys", "2^25-keys"])
def test_gathered_radix_end(ls, torch_gpu, n, outputs, V):
    """GS_MAX_N = 2^25 keys and one fewer, u32: the keys-only inner sort runs the gathered radix for
    the last time at 2^25 - 1 and onesweep from 2^25; the key/value sort runs onesweep with payloads
    on both sides (api.hip), where the workspace layout still changes (uq_inner_bytes).  The keys are
    spread(n, V): V distinct full-width values in turn, whose expectation is a closed form that
    sorts V values, not n."""
    assert n in (ls.GS_MAX_N - 1, ls.GS_MAX_N) and ls.GS_MAX_N == 1 << 25
    x, exp = U.spread(n, V, "u32"), U.spread_expected(n, V, "u32")
    assert exp[4] == V
    route = run_routed(ls, torch_gpu, x, "u32", outputs, exp, f"spread V={V}")
    assert route == ("onesweep" if outputs == ALL or n == ls.GS_MAX_N else "gather")


# ---- ls.unique on views ----------------------------------------------------------------------------------
PY_DTYPES = [("int32", "i32"), ("float32", "f32"), ("int64", "i64"), ("float64", "f64"), ("uint32", "u32"), ("uint64", "u64")]


@pytest.mark.parametrize("name,kind", PY_DTYPES, ids=[d for d, _ in PY_DTYPES])
def test_python_views_and_dtypes(ls, torch_gpu, name, kind):
    """ls.unique on x[1:], a contiguous view of 2C + 3 elements that starts one element into its
    allocation, with a caller's workspace that serves three calls: every output in sorted mode, every
    output in consecutive mode, the values alone.  Against the model on the words; the integer dtypes
    against torch.unique and torch.unique_consecutive (on the host, as int64 or by the words' order)
    as well.  A dtype that this torch does not have has nothing to run."""
    torch = torch_gpu
    if not hasattr(torch, name):
        return
    dtype, n = getattr(torch, name), 2 * chunk(ls) + 3
    esize = 8 if kind in U.KINDS64 else 4
    raw = torch.int64 if esize == 8 else torch.int32
    words = lambda t: t.view(raw).cpu().numpy().view(U.word_dtype(kind))  # noqa: E731

    def view_of(x):
        store = torch.from_numpy(signed(np.concatenate([x[:1], x])).copy()).cuda().view(dtype)
        v = store[1:]
        assert v.data_ptr() % 16 == esize and v.is_contiguous() and v.numel() == n and v.dtype == dtype
        return v

    ws = torch.full((max(ls.unique_workspace_bytes(n, kind, c, True) for c in (False, True)),), 0xCD, dtype=torch.uint8,
                    device="cuda")
    xs = U.generate("mod1000", n, 0x9107, kind)
    xc = U.from_ints(np.arange(n, dtype=np.int64) // 3 % 11, kind)
    for x, consecutive in ((xs, False), (xc, True)):
        v = view_of(x)
        values, inverse, counts, index = ls.unique(v, return_inverse=True, return_counts=True, return_index=True,
                                                   consecutive=consecutive, workspace=ws)
        ev, ec, ef, ei, m = U.expected(x, kind, consecutive)
        assert values.dtype == dtype and inverse.dtype == counts.dtype == index.dtype == torch.int32
        assert values.numel() == counts.numel() == index.numel() == m and inverse.numel() == n
        for what, got, want in (("values", values, ev), ("counts", counts, ec), ("index", index, ef), ("inverse", inverse, ei)):
            got = got.view(raw).cpu().numpy().view(want.dtype) if what == "values" else got.cpu().numpy().view(np.uint32)
            np.testing.assert_array_equal(got, want, err_msg=f"{what}: {name} consecutive={consecutive}")
        np.testing.assert_array_equal(words(v), x, err_msg="the input was written")
        if kind in U.INT_KINDS:
            # an order-preserving map of the keys into int64 (uint64: by rank), so torch's own kernels take them
            ints = {"i32": lambda w: w.view(np.int32).astype(np.int64), "u32": lambda w: w.astype(np.int64),
                    "i64": lambda w: w.view(np.int64), "u64": lambda w: np.searchsorted(np.unique(x), w).astype(np.int64)}[kind]
            t = torch.from_numpy(ints(x).copy())
            if consecutive:
                tv, ti, tc = torch.unique_consecutive(t, return_inverse=True, return_counts=True)
            else:
                tv, ti, tc = torch.unique(t, sorted=True, return_inverse=True, return_counts=True)
            np.testing.assert_array_equal(ints(words(values)), tv.numpy())
            np.testing.assert_array_equal(inverse.cpu().numpy(), ti.numpy())
            np.testing.assert_array_equal(counts.cpu().numpy(), tc.numpy())
    only = ls.unique(view_of(xs), workspace=ws)
    assert isinstance(only, torch.Tensor) and only.dtype == dtype
    np.testing.assert_array_equal(words(only), U.expected(xs, kind)[0])
