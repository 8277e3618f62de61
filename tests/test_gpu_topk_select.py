"""The radix select of labsort_topk_device on the GPU where test_gpu_topk.py does not reach: rows of
more than 1024 chunks (a histogram workgroup counts several chunks, the scan over the chunks takes a
second step and carries its sums), every level at which a row can narrow and both sides of the
candidate buffer's capacity, rows of all those kinds in one call and in one replayed graph, rows at
every misalignment of the kernels' 16-byte group loads, and a seeded sweep over key types, directions, shapes, paths and options.

Every call follows test_gpu_topk.py's protocol: a workspace filled with 0xFF, outputs filled with a
pattern, the status call afterwards, the input unchanged, whole key and position arrays compared
exactly (float keys: NaN-ness equal, everything else bit-exact) with tests/topk_model.py.  Cases (a)
to (c) first assert on the host that the call runs the select and that each row narrows at the
level the case is about (topk_model.narrow_level): a case cannot pass through another path."""
import functools

import numpy as np
import pytest

import f16_model as M16
import f32_model as M32
import topk_model as T

pytestmark = pytest.mark.gpu

C = T.constants()
CHUNK, BLOCK = C["TK_CHUNK"], C["TK_BLOCK"]
BOTH = [False, True]
NEVER = T.NEVER

# One chunk more than the histogram workgroups of a row, and five keys: 1026 chunks, two per histogram
# workgroup, a last chunk of five keys, and a scan of one full step and a step of two chunks.
LONG = (C["TK_MAX_HIST_WG"] + 1) * CHUNK + 5
MCOLS = 70001  # odd: row 1 starts off a 16-byte boundary; the candidate buffer holds 8750 pairs
MKS = (1, 65, 1000)  # and MCOLS // TOPK_SORT_DIV


def torch_dtype(torch, kind):
    return {"u32": torch.int32, "i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]


def run(ls, torch, x, k, kind, largest, ws=None, with_idx=True, in_off=0, aligned=False):
    """in_off: elements between the start of the storage and the matrix.  aligned: the case relies on
    the matrix starting on a 16-byte boundary."""
    rows, cols = x.shape
    wide = T.bits_of(kind) == 32
    it, ut = (torch.int32, np.uint32) if wide else (torch.int16, np.uint16)
    st = np.int32 if wide else np.int16
    assert x.dtype == ut
    store = torch.full((rows * cols + in_off,), 0x1111, dtype=it, device="cuda")
    d = store[in_off:].view(rows, cols)
    d.copy_(torch.from_numpy(x.view(st).copy()))  # (a copy: shared inputs are read-only)
    assert not aligned or d.data_ptr() % 16 == 0
    before = store.clone()
    ostore = torch.full((rows * k + 1,), 0x5A5A, dtype=it, device="cuda")
    ko = ostore[:rows * k].view(rows, k)
    io = torch.full((rows, k), -7, dtype=torch.int32, device="cuda") if with_idx else None
    if ws is None:
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.numel() >= ls.topk_workspace_bytes(rows, cols, k)
    dt = torch_dtype(torch, kind)
    ls.topk_device(d.view(dt), rows, cols, k, ko.view(dt), io, largest=largest, key=kind, workspace=ws)
    ls.topk_workspace_status(ws)
    assert torch.equal(store, before), "the input was written"
    assert int(ostore[-1]) == 0x5A5A, "written past the output"
    return ko.cpu().numpy().view(ut), (io.cpu().numpy().view(np.uint32) if with_idx else None)


def check(ls, torch, x, k, kind, largest, want=None, **kw):
    ek, ei = want if want is not None else T.expected(x, k, kind, largest)
    gk, gi = run(ls, torch, x, k, kind, largest, **kw)
    msg = f"{kind} {x.shape} k={k} largest={largest}"
    T.assert_keys(gk, ek, kind, msg)
    if gi is not None:
        np.testing.assert_array_equal(gi, ei, err_msg=f"positions {msg}")
    return gk, gi


def assert_select_narrows(ls, x, k, kind, largest, levels):
    """The host-side condition of a case: the select runs, and row r narrows after levels[r]."""
    rows, cols = x.shape
    assert cols > ls.segment_pair_tile_keys() and T.select_runs(cols, k, ls.TOPK_SORT_DIV), (cols, k)
    u = T.u_of(x, kind, largest)
    got = [T.narrow_level(u[r], k, T.cap_of(cols, C), T.levels_of(kind)) for r in range(rows)]
    assert got == list(levels), f"{kind} {x.shape} k={k} largest={largest}: rows narrow after {got}, the case is about {list(levels)}"
    return u


def frozen(x):
    x.setflags(write=False)
    return x


def rand32(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


# ---- a. rows past 1024 chunks ----

def test_long_shape():
    nch = -(-LONG // CHUNK)
    g = -(-nch // C["TK_MAX_HIST_WG"])
    assert LONG == 16793605 and nch == C["TK_MAX_HIST_WG"] + 2 and g == 2 and LONG % CHUNK == 5
    assert nch - BLOCK == 2  # the scan: one full step, then the last two chunks


@functools.lru_cache(maxsize=1)
def long_uniform():
    return frozen(rand32((1, LONG), 0x70F0))


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("k", [1, 1000])
def test_long_int32_uniform(ls, torch_gpu, k, largest):
    x = long_uniform()
    assert_select_narrows(ls, x, k, "i32", largest, [0])
    check(ls, torch_gpu, x, k, "i32", largest)


def test_long_uint32_mod1000_never_narrows(ls, torch_gpu):
    """Every level counts the raw input with two chunks per workgroup and scans in two steps; the
    final compaction reads the raw input."""
    x = long_uniform() % np.uint32(1000)
    assert_select_narrows(ls, x, 20000, "u32", False, [NEVER])
    check(ls, torch_gpu, x, 20000, "u32", False)


@pytest.mark.parametrize("narrows", ["level0", "never"])
def test_long_ties_across_the_scan_carry(ls, torch_gpu, narrows):
    """100 small keys, then 11 equal keys V around the chunk at which the scan starts its second
    step; k = 106 takes the first six of them.  level0: the candidate buffer is filled through
    eqbase across the carry; never: the final pass places the keys through lowbase and eqbase."""
    b = BLOCK * CHUNK
    assert b + 6 <= LONG
    if narrows == "level0":
        V = 1000
        x = long_uniform() | np.uint32(0x80000000)
    else:
        V = 0x5A5A5A00
        x = np.uint32(V) | (long_uniform() % np.uint32(255) + np.uint32(1))
    x[0, 100:200] = np.arange(100, dtype=np.uint32)
    x[0, b - 5:b + 6] = V
    assert np.count_nonzero(x == V) == 11 and np.count_nonzero(x < V) == 100
    assert_select_narrows(ls, x, 106, "u32", False, [0 if narrows == "level0" else NEVER])
    gk, gi = check(ls, torch_gpu, x, 106, "u32", False)
    assert list(gi[0, 100:]) == list(range(b - 5, b + 1)) and np.all(gk[0, 100:] == V)
    np.testing.assert_array_equal(gi[0, :100], np.arange(100, 200))


def test_long_float32_normals(ls, torch_gpu):
    x = M32.normal_words((1, LONG), 0x70F1)
    assert_select_narrows(ls, x, 1024, "f32", True, [0])
    check(ls, torch_gpu, x, 1024, "f32", True)


@pytest.mark.parametrize("kind", T.KINDS16)
def test_long_16bit_rows(ls, torch_gpu, kind):
    """Row 0 normals, row 1 heavy ties with NaNs (largest first, the k-th key is a NaN; the NaNs are a
    tenth of the row, so both narrow after level 0), row 2 keys sharing their top byte, which never
    narrows: level 1 and the final pass read the raw 16-bit input.  With positions and without."""
    x = np.stack([M16.normal_words((LONG,), 0x70F2, kind), M16.tie_words((LONG,), 0x70F3, kind),
                  T.raw_of(T.row_narrowing_at(NEVER, LONG, 0x70F4, 16), kind, True)])
    assert_select_narrows(ls, x, 1024, kind, True, [0, 0, NEVER])
    want = T.expected(x, 1024, kind, True)
    check(ls, torch_gpu, x, 1024, kind, True, want=want)
    check(ls, torch_gpu, x, 1024, kind, True, want=want, with_idx=False)


# ---- b. the narrowing matrix ----

def matrix_rows(kind, largest, k, seed):
    """(words, the level each row narrows after, the rows whose bucket fills the candidate buffer)."""
    bits, cap, kb = T.bits_of(kind), T.cap_of(MCOLS, C), T.k_below_of(k)
    if bits == 32:
        plan = [("at", 0), ("at", 1), ("at", 2), ("at", NEVER), (cap, 0), (cap + 1, 0), (cap, 1), (cap + 1, 1)]
        levels = [0, 1, 2, NEVER, 0, 1, 1, 2]
    else:
        plan = [("at", 0), ("at", NEVER), (cap, 0), (cap + 1, 0)]
        levels = [0, NEVER, 0, NEVER]
    u = np.stack([T.row_narrowing_at(lv, MCOLS, seed + i, bits) if what == "at" else T.row_bucket_of(what, lv, MCOLS, kb, seed + i, bits)
                  for i, (what, lv) in enumerate(plan)])
    return T.raw_of(u, kind, largest), levels, [i for i, (what, _) in enumerate(plan) if what == cap]


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("kind", T.KINDS)
def test_narrowing_matrix(ls, torch_gpu, kind, largest):
    """One call per k over rows that narrow after level 0, 1, 2 and never, and rows whose bucket
    holds exactly the candidate buffer's capacity (filled to its last slot) or one key more (the
    row must not narrow there), each bucket row with the same number of keys below its bucket."""
    assert T.cap_of(MCOLS, C) == 8750 and (MCOLS * (T.bits_of(kind) // 8)) % 16
    for k in MKS + (MCOLS // ls.TOPK_SORT_DIV,):
        x, levels, full = matrix_rows(kind, largest, k, 0x7100 + k)
        u = assert_select_narrows(ls, x, k, kind, largest, levels)
        _, gi = check(ls, torch_gpu, x, k, kind, largest)
        for r in full:  # of the k-th key's ties, the first in position order are taken
            kth = np.partition(u[r], k - 1)[k - 1]
            nlt, ties = int(np.count_nonzero(u[r] < kth)), np.flatnonzero(u[r] == kth)
            assert nlt < k <= nlt + ties.size and ties.size > 1
            np.testing.assert_array_equal(gi[r, nlt:], ties[:k - nlt], err_msg=f"ties taken, row {r} k={k}")


# ---- b2. every misalignment of the group loads ----

ACOLS = CHUNK + 9


@functools.lru_cache(maxsize=None)
def misaligned_rows(bits, level):
    """Eight rows of ACOLS order images that narrow after `level` (0 or NEVER), read-only."""
    return frozen(np.stack([T.row_narrowing_at(level, ACOLS, 0x7300 + r, bits) for r in range(8)]))


@pytest.mark.parametrize("largest", BOTH)
@pytest.mark.parametrize("kind", ["i32", "f32", "bf16", "f16"])
def test_every_group_misalignment(ls, torch_gpu, kind, largest):
    """Eight rows of TK_CHUNK + 9 keys behind a 16-byte aligned base.  The width is odd, so row r
    starts r elements into its 16 bytes: every misalignment 0 .. 7 of the loads of eight 16-bit keys
    and, twice, all four of the loads of four words.  The second chunk is nine keys: a head, a tail
    and at most two whole groups.  Two inputs per key type: rows that narrow after level 0, so every
    later read is a read of the candidate buffer in quads (of a 16-bit call too), and rows that never
    narrow, so every level and the final compaction read the raw input."""
    assert ACOLS % 8 == 1 and -(-ACOLS // CHUNK) == 2
    for level in (0, NEVER):
        x = T.raw_of(misaligned_rows(T.bits_of(kind), level), kind, largest)
        assert_select_narrows(ls, x, 5, kind, largest, [level] * 8)
        check(ls, torch_gpu, x, 5, kind, largest, aligned=True)


# ---- c. graph replay across levels ----

def test_graph_replay_across_levels(ls, torch_gpu):
    """One captured call replayed on four inputs that rotate the four rows through narrowing after
    level 0, 1, 2 and never, so every row changes its level on every replay; then constant keys."""
    torch = torch_gpu
    rows, cols, k, order = 4, MCOLS, 500, [0, 1, 2, NEVER]
    src = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    ko = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    io = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
    ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.topk_device(src, rows, cols, k, ko, io, key="i32", workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.topk_device(src, rows, cols, k, ko, io, key="i32", workspace=ws, stream=torch.cuda.current_stream())
    inputs = []
    for i in range(4):
        levels = [order[(r + i) % 4] for r in range(rows)]
        x = T.raw_of(np.stack([T.row_narrowing_at(lv, cols, 0x7200 + 4 * i + r) for r, lv in enumerate(levels)]), "i32")
        assert_select_narrows(ls, x, k, "i32", False, levels)
        inputs.append((f"replay {i}: levels {levels}", x))
    assert all(len({T.narrow_level(T.u_of(x, "i32")[r], k, T.cap_of(cols, C), 4) for _, x in inputs}) == 4 for r in range(rows))
    const = np.full((rows, cols), 0x80000001, dtype=np.uint32)
    assert_select_narrows(ls, const, k, "i32", False, [NEVER] * rows)
    inputs.append(("constant keys", const))
    for name, x in inputs:
        src.copy_(torch.from_numpy(x.view(np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.topk_workspace_status(ws)
        ek, ei = T.expected(x, k, "i32", False)
        np.testing.assert_array_equal(ko.cpu().numpy().view(np.uint32), ek, err_msg=name)
        np.testing.assert_array_equal(io.cpu().numpy().view(np.uint32), ei, err_msg=name)
        np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x, err_msg=f"the input was written, {name}")


# ---- d. the seeded sweep ----

@pytest.mark.parametrize("seed", T.SWEEP_SEEDS)
def test_seeded_sweep(ls, torch_gpu, seed):
    """40 cases per seed (topk_model.sweep_case): 1 to 6 rows of tile < cols <= 2^18 keys, a third of
    the widths at a chunk edge, k log-uniform in 1 .. cols (the select and whole-row sorting), the five
    key types, both directions, with and without positions, the input at the start of its storage
    or one element in, every row from its own generator.  One workspace per seed, filled with 0xFF
    once and never cleared between the cases."""
    torch = torch_gpu
    cases = list(T.sweep_cases(seed, ls.segment_pair_tile_keys(), C, ls.TOPK_SORT_DIV))
    size = max(ls.topk_workspace_bytes(c["rows"], c["cols"], c["k"]) for c in cases)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    failures, paths, levels = [], {}, {}
    for i, c in enumerate(cases):
        paths[c["path"]] = paths.get(c["path"], 0) + 1
        for lv in c["levels"] or ():
            levels[lv] = levels.get(lv, 0) + 1
        try:
            check(ls, torch, c["x"], c["k"], c["kind"], c["largest"], ws=ws, with_idx=c["with_idx"], in_off=c["in_off"])
        except AssertionError as e:
            failures.append(f"seed {seed} case {i}: {c['tag']}: {str(e).strip().splitlines()[0]}")
    print(f"seed {seed}: paths {paths}, narrowing levels of the select's rows {levels}")
    assert not failures, failures
