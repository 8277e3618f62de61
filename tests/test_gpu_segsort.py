"""Segmented sort on the GPU (labsort_sort_segments_device / _pairs_device): every segment
[offsets[i], offsets[i+1]) sorted on its own, on the LDS path (max_segment_keys up to the
tile) and on the general path, against numpy: per-segment np.sort and, for pairs,
per-segment np.argsort(kind="stable").  Whole output arrays are compared, so any bleed
between neighbouring segments shows.  Every case ends with segments_workspace_status."""
import numpy as np
import pytest

import sort_sweep_model as S

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A


def offsets_of(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.uint32)


def expect(keys, offs, key, vals=None):
    """keys / vals: uint32 arrays.  Per-segment np.sort, or np.argsort(kind="stable") for pairs."""
    typed = keys.view(np.int32) if key == "i32" else keys
    ek = np.empty_like(keys)
    ev = None if vals is None else np.empty_like(vals)
    o = [int(x) for x in offs]
    for a, b in zip(o[:-1], o[1:]):
        if b - a == 0:
            continue
        if vals is None:
            ek[a:b] = np.sort(typed[a:b]).view(np.uint32)
        else:
            order = np.argsort(typed[a:b], kind="stable")
            ek[a:b] = keys[a:b][order]
            ev[a:b] = vals[a:b][order]
    return ek, ev


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def zeros_ws(ls, torch, n, nseg, m, pairs):
    return torch.zeros(max(ls.segments_workspace_bytes(n, nseg, m, pairs), 256), dtype=torch.uint8, device="cuda")


def run(ls, torch, keys, offs, m, key="u32", vals=None, inplace=False, ws=None):
    """One call + status; returns the outputs as uint32 arrays."""
    n, nseg, pairs = keys.size, offs.size - 1, vals is not None
    dk, do = dev(torch, keys), dev(torch, offs)
    if ws is None:
        ws = zeros_ws(ls, torch, n, nseg, m, pairs)
    ok = dk if inplace else torch.full_like(dk, PATTERN)
    ov = None
    if pairs:
        dv = dev(torch, vals)
        ov = dv if inplace else torch.full_like(dv, PATTERN)
        ls.sort_segments_pairs_device(dk, dv, ok, ov, n, do, nseg, m, key=key, workspace=ws)
    else:
        ls.sort_segments_device(dk, ok, n, do, nseg, m, key=key, workspace=ws)
    ls.segments_workspace_status(ws)
    return ok.cpu().numpy().view(np.uint32), (ov.cpu().numpy().view(np.uint32) if pairs else None)


def check(ls, torch, keys, offs, m, key="u32", vals=None, inplace=False):
    gk, gv = run(ls, torch, keys, offs, m, key, vals, inplace)
    ek, ev = expect(keys, offs, key, vals)
    np.testing.assert_array_equal(gk, ek)
    if vals is not None:
        np.testing.assert_array_equal(gv, ev)


def rand_u32(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def tile(ls, pairs):
    return ls.segment_pair_tile_keys() if pairs else ls.segment_tile_keys()


# ---- 1. every short length ----------------------------------------------------------------
@pytest.mark.parametrize("m", [300, 0])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("key", ["u32", "i32"])
def test_every_short_length(ls, torch_gpu, key, pairs, m):
    rng = np.random.default_rng(1)
    offs = offsets_of(range(301))
    assert offs[-1] == 45150
    keys = rand_u32(rng, 45150)
    vals = rand_u32(rng, 45150) if pairs else None
    check(ls, torch_gpu, keys, offs, m, key, vals)


# ---- 2. both sides of every class edge ----------------------------------------------------
@pytest.mark.parametrize("ei", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("pairs", [False, True])
def test_class_edges(ls, torch_gpu, pairs, ei):
    edges = ls.segment_class_edges(pairs)
    if ei >= len(edges):
        ei = len(edges) - 1
    E = edges[ei]
    # E - 1 keys first: the next segments start at odd word offsets
    lengths = [E - 1, 0, E, 1, E + 1, 0, 1, 1, E, E + 1, 0, E - 1]
    offs = offsets_of(lengths)
    assert any(int(o) % 4 for o in offs[:-1])
    rng = np.random.default_rng(20 + ei)
    n = int(offs[-1])
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n) if pairs else None
    # E + 1 past the last edge is longer than the tile: the general path
    check(ls, torch_gpu, keys, offs, E + 1, "u32", vals)
    check(ls, torch_gpu, keys, offs, E + 1, "i32", vals)


# ---- 3. stability --------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "general"])
@pytest.mark.parametrize("dist", ["mod4", "const"])
def test_stability(ls, torch_gpu, dist, path):
    e = ls.segment_class_edges(True)
    T = e[-1]
    lengths = list(range(301))
    for E in e[:-1]:
        lengths += [E - 1, E, E + 1]
    lengths += [T - 1, T] + ([T + 1] if path == "general" else [])
    offs = offsets_of(lengths)
    n = int(offs[-1])
    rng = np.random.default_rng(3)
    keys = (rand_u32(rng, n) % 4).astype(np.uint32) if dist == "mod4" else np.full(n, 0xC0FFEE, dtype=np.uint32)
    vals = np.arange(n, dtype=np.uint32)  # the global index
    check(ls, torch_gpu, keys, offs, T if path == "lds" else 0, "u32", vals)


# ---- 4. maximum keys against the padding ---------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("key", ["u32", "i32"])
def test_max_keys_against_padding(ls, torch_gpu, key, pairs):
    lengths = [1, 63, 65, 100, 257, 4097]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    rng = np.random.default_rng(4)
    if key == "u32":
        keys = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    else:  # the largest int32 and -1 (all ones)
        keys = np.where(rng.integers(0, 2, size=n) == 1, 0x7FFFFFFF, 0xFFFFFFFF).astype(np.uint32)
    few = rng.random(n) < 0.05
    keys[few] = rand_u32(rng, int(few.sum()))
    keys[0] = 0xFFFFFFFF if key == "u32" else 0x7FFFFFFF  # the 1-key segment holds the maximum
    vals = (np.arange(n, dtype=np.uint32) + 1) if pairs else None  # non-zero: padding carries payload 0
    m = 4097 if 4097 <= tile(ls, pairs) else 0
    gk, gv = run(ls, torch_gpu, keys, offs, m, key, vals)
    ek, ev = expect(keys, offs, key, vals)
    np.testing.assert_array_equal(gk, ek)
    if pairs:
        assert np.all(gv != 0)
        np.testing.assert_array_equal(gv, ev)


# ---- 5. in place ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "general"])
@pytest.mark.parametrize("pairs", [False, True])
def test_in_place(ls, torch_gpu, pairs, path):
    T = tile(ls, pairs)
    lengths = [0, 1, 2, 17, 64, 65, 255, 256, 257, 1000, 4096, 4097, 3, T, 1, 0, T - 1, 5000, 300, 7]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    rng = np.random.default_rng(5)
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n) if pairs else None
    check(ls, torch_gpu, keys, offs, T if path == "lds" else 0, "i32", vals, inplace=True)


# ---- 6. general path -----------------------------------------------------------------------
@pytest.mark.parametrize("promise", ["unknown", "true_max"])
@pytest.mark.parametrize("pairs", [False, True])
def test_general_path_long_segments(ls, torch_gpu, pairs, promise):
    T = tile(ls, pairs)
    lengths = [T + 1, 5, 0, 2 * T + 3, 1]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    rng = np.random.default_rng(6)
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n) if pairs else None
    m = 0 if promise == "unknown" else max(lengths)
    check(ls, torch_gpu, keys, offs, m, "u32", vals)
    check(ls, torch_gpu, keys, offs, m, "i32", vals)


@pytest.mark.parametrize("pairs", [False, True])
def test_general_path_radix_inner_sort(ls, torch_gpu, pairs):
    """2^18 + 4099 keys: past the pair sorts' merge bound, so the inner sorts run their radix"""
    T = tile(ls, pairs)
    n = (1 << 18) + 4099
    rng = np.random.default_rng(66)
    lengths = []
    while sum(lengths) < n:
        lengths.append(min(int(rng.integers(0, 3 * T + 1)), n - sum(lengths)))
    offs = offsets_of(lengths)
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n) if pairs else None
    check(ls, torch_gpu, keys, offs, 0, "u32", vals)
    check(ls, torch_gpu, keys, offs, max(max(lengths), T + 1), "i32", vals)


# ---- 7. more segments than any resident grid -----------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
def test_many_tiny_segments(ls, torch_gpu, pairs):
    rng = np.random.default_rng(7)
    lengths = rng.integers(1, 3, size=300000)
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n) if pairs else None
    check(ls, torch_gpu, keys, offs, 2, "u32", vals)


@pytest.mark.parametrize("shape", ["tile_class", "block_class", "long_wave_class"])
def test_many_segments_per_grid(ls, torch_gpu, shape):
    e = ls.segment_class_edges(False)
    assert len(e) >= 3
    # 600 segments one key past the block-class edge (tile class: one workgroup per CU), and more
    # segments of the block class and of the longest wave class than their grids hold
    nseg, length = {"tile_class": (600, e[-2] + 1), "block_class": (1700, e[-3] + 1),
                    "long_wave_class": (9000, e[0] + 1)}[shape]
    offs = offsets_of([length] * nseg)
    n = int(offs[-1])
    rng = np.random.default_rng(77)
    keys = rand_u32(rng, n)
    gk, _ = run(ls, torch_gpu, keys, offs, length, "u32")
    np.testing.assert_array_equal(gk, np.sort(keys.reshape(nseg, length), axis=1).reshape(-1))


# ---- 8. rejected offsets -------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("bad,path", [("decrease", "lds"), ("first", "lds"), ("last", "lds"), ("too_long", "lds"),
                                      ("decrease", "general"), ("first", "general"), ("last", "general")])
def test_rejected_offsets(ls, torch_gpu, bad, path, pairs):
    torch = torch_gpu
    lengths = [10, 0, 300, 1, 64, 5000, 2, 100]
    good = offsets_of(lengths)
    n, nseg = int(good[-1]), len(lengths)
    m = 5000 if path == "lds" else 0
    offs = good.copy()
    if bad == "decrease":
        offs[3] = offs[2] - 1  # ... 10, 9, 311 ...: decreases once
    elif bad == "first":
        offs[0] = 1
    elif bad == "last":
        offs[nseg] = n - 1
    else:
        m = 4999  # the 5000-key segment is one key longer than promised
    rng = np.random.default_rng(8)
    keys = rand_u32(rng, n)
    vals = rand_u32(rng, n)
    dk, dv, do = dev(torch, keys), dev(torch, vals), dev(torch, offs)
    ok, ov = torch.full_like(dk, PATTERN), torch.full_like(dv, PATTERN)
    ws = zeros_ws(ls, torch, n, nseg, max(m, 5000) if path == "lds" else 0, pairs)

    def call(offsets, mm):
        if pairs:
            ls.sort_segments_pairs_device(dk, dv, ok, ov, n, offsets, nseg, mm, workspace=ws)  # returns OK
        else:
            ls.sort_segments_device(dk, ok, n, offsets, nseg, mm, workspace=ws)

    call(do, m)
    with pytest.raises(ls.LabsortError) as ei:
        ls.segments_workspace_status(ws)
    assert ei.value.status == ls.ERR_ARG
    # the sort kernels returned at the error word: the outputs still hold the pattern
    assert bool((ok == PATTERN).all())
    if pairs:
        assert bool((ov == PATTERN).all())
    # a valid call on the same workspace afterwards succeeds
    call(dev(torch, good), 5000 if path == "lds" else 0)
    ls.segments_workspace_status(ws)
    ek, ev = expect(keys, good, "u32", vals if pairs else None)
    np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32), ek)
    if pairs:
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), ev)


# ---- 9. graph replay on new keys and new offsets -------------------------------------------
def _graph_lengths(rng, n, nseg, T):
    """nseg lengths summing to n: a few up to the tile, some block class, many short, empties"""
    lengths = [int(rng.integers(4097, T + 1)) for _ in range(3)] + [int(rng.integers(257, 4097)) for _ in range(20)]
    while sum(lengths) < n:
        lengths.append(min(int(rng.integers(0, 257)), n - sum(lengths)))
    assert sum(lengths) == n and len(lengths) <= nseg
    lengths += [0] * (nseg - len(lengths))
    return rng.permutation(np.asarray(lengths))


@pytest.mark.parametrize("path", ["lds", "general"])
@pytest.mark.parametrize("pairs", [False, True])
def test_segments_graph_replay(ls, torch_gpu, pairs, path):
    torch = torch_gpu
    n, nseg = 200_000, 2048
    T = tile(ls, pairs)
    m = T if path == "lds" else 0
    rng = np.random.default_rng(9)
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    vsrc = torch.empty(n, dtype=torch.int32, device="cuda")
    out, vout = torch.empty_like(src), torch.empty_like(vsrc)
    offs = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    ws = zeros_ws(ls, torch, n, nseg, m, pairs)

    def load(seed):
        r = np.random.default_rng(seed)
        o = offsets_of(_graph_lengths(r, n, nseg, T))
        k, v = rand_u32(r, n), rand_u32(r, n)
        if seed & 1:
            k = (k % 1000).astype(np.uint32)
        src.copy_(dev(torch, k))
        vsrc.copy_(dev(torch, v))
        offs.copy_(dev(torch, o))
        return k, v, o

    def call(stream):
        if pairs:
            ls.sort_segments_pairs_device(src, vsrc, out, vout, n, offs, nseg, m, key="i32", workspace=ws, stream=stream)
        else:
            ls.sort_segments_device(src, out, n, offs, nseg, m, key="i32", workspace=ws, stream=stream)

    load(int(rng.integers(1 << 30)))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        call(s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream())
    for seed in (0x5E65001, 0x5E65002):
        k, v, o = load(seed)
        out.fill_(PATTERN)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.segments_workspace_status(ws)
        ek, ev = expect(k, o, "i32", v if pairs else None)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ek)
        if pairs:
            np.testing.assert_array_equal(vout.cpu().numpy().view(np.uint32), ev)


# ---- 10. seeded stress ---------------------------------------------------------------------
def test_segments_seeded_stress(ls, torch_gpu):
    rng = np.random.default_rng(0x5E6)
    dists = ["u32", "mod100", "const", "sorted", "reversed"]
    for case in range(100):
        n = int(rng.integers(0, (1 << 17) + 1)) if case else 0
        if case == 1:
            n = 1 << 17
        nseg = int(rng.integers(1, 2000)) if case % 3 else int(rng.integers(1, 12))
        cuts = np.sort(rng.integers(0, n + 1, size=nseg - 1))  # duplicates: empty segments
        offs = np.concatenate(([0], cuts, [n])).astype(np.uint32)
        dist = dists[case % 5]
        if dist == "u32":
            keys = rand_u32(rng, n)
        elif dist == "mod100":
            keys = (rand_u32(rng, n) % 100).astype(np.uint32)
        elif dist == "const":
            keys = np.full(n, 0x80000000, dtype=np.uint32)
        else:
            keys = np.sort(rand_u32(rng, n))
            if dist == "reversed":
                keys = keys[::-1].copy()
        key = "i32" if (case // 5) % 2 else "u32"
        pairs = bool((case // 10) % 2)
        inplace = bool((case // 20) % 2)
        true_max = int(np.diff(offs.astype(np.int64)).max())
        m = true_max if rng.integers(0, 2) else 0
        vals = rand_u32(rng, n) if pairs else None
        gk, gv = run(ls, torch_gpu, keys, offs, m, key, vals, inplace)
        ek, ev = expect(keys, offs, key, vals)
        tag = f"case {case}: n={n} nseg={nseg} {dist} {key} pairs={pairs} inplace={inplace} m={m}"
        np.testing.assert_array_equal(gk, ek, err_msg=tag)
        if pairs:
            np.testing.assert_array_equal(gv, ev, err_msg=tag)


# ---- 10b. the pass-skip logic: every set of differing digits ---------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("key", ["u32", "i32"])
def test_digit_masks(ls, torch_gpu, key, pairs):
    """Segments of 1 to 9000 keys and of the tile's length, each length once per set of differing
    digits (16 masks) and per variant of sort_sweep_model.digit_mask_rows (digits random per key, two
    values one bit apart, all keys equal but the first, the last or one in the middle; at the tile's
    length three of the five): k_seg_wave's own copy of the skip test and the block kernels'.  The
    payloads are the global index, so equal keys must keep their order whichever passes ran."""
    T = tile(ls, pairs)
    keys, offs, labels = S.mask_segments(key, T, 0x5E60)
    n = keys.size
    assert n < 4_000_000 and max(length for length, _, _ in labels) == T
    vals = np.arange(n, dtype=np.uint32) if pairs else None
    gk, gv = run(ls, torch_gpu, keys, offs, T, key, vals)
    ek, ev = expect(keys, offs, key, vals)
    wrong = gk != ek
    if pairs:
        wrong |= gv != ev
    if wrong.any():
        s = int(np.searchsorted(offs.astype(np.int64), int(np.flatnonzero(wrong)[0]), side="right")) - 1
        raise AssertionError(f"{key} pairs={pairs}: {int(wrong.sum())} elements differ, the first in segment {s}: "
                             f"{labels[s][0]} keys, mask {labels[s][1]:#x} {labels[s][2]}")


# ---- 11. timing hook -----------------------------------------------------------------------
def test_segsort_timing_hook(ls, torch_gpu):
    rng = np.random.default_rng(11)
    offs = offsets_of([100] * 50)
    keys = rand_u32(rng, 5000)
    ls.timing_enable(True)
    try:
        gk, _ = run(ls, torch_gpu, keys, offs, 100)
        ms, launches = ls.timing_read("segsort")
    finally:
        ls.timing_enable(False)
    assert launches > 0 and ms >= 0.0
    np.testing.assert_array_equal(gk, np.sort(keys.reshape(50, 100), axis=1).reshape(-1))


def test_row_offsets(ls, torch_gpu):
    o = ls.row_offsets(7, 33)
    assert o.dtype == torch_gpu.int32 and o.is_cuda
    np.testing.assert_array_equal(o.cpu().numpy(), np.arange(8) * 33)
