"""Segmented sort with float32 keys on the GPU (labsort_sort_segments_device / _pairs_device, key type
F32), LDS path and general path, against the numpy model of the contract (tests/f32_model.py): each
segment's stable argsort of ord(key).  Keys compare NaN-ness everywhere and bit-exact otherwise,
payloads exactly; whole output arrays are compared, so bleed between segments shows.  Every call
runs on a workspace filled with 0xFF and outputs filled with a pattern, is followed by the status
call, and an out-of-place call must leave its input as it was."""
import numpy as np
import pytest

import f32_model as M
import sort_sweep_model as S

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
NAN_WORDS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)


def offsets_of(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.uint32)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def ff_ws(ls, torch, n, nseg, m, pairs):
    return torch.full((max(ls.segments_workspace_bytes(n, nseg, m, pairs), 256),), 0xFF, dtype=torch.uint8, device="cuda")


def run(ls, torch, keys, offs, m, vals=None, inplace=False):
    n, nseg, pairs = keys.size, offs.size - 1, vals is not None
    dk, do = dev(torch, keys), dev(torch, offs)
    before = dk.clone()
    ws = ff_ws(ls, torch, n, nseg, m, pairs)
    ok = dk if inplace else torch.full_like(dk, PATTERN)
    ov = None
    fk, fo = dk.view(torch.float32), ok.view(torch.float32)  # float32 tensors over the same words
    if pairs:
        dv = dev(torch, vals)
        vbefore = dv.clone()
        ov = dv if inplace else torch.full_like(dv, PATTERN)
        ls.sort_segments_pairs_device(fk, dv, fo, ov, n, do, nseg, m, key="f32", workspace=ws)
    else:
        ls.sort_segments_device(fk, fo, n, do, nseg, m, key="f32", workspace=ws)
    ls.segments_workspace_status(ws)
    if not inplace:
        assert torch.equal(dk, before), "the input keys were written"
        if pairs:
            assert torch.equal(dv, vbefore), "the input payloads were written"
    return ok.cpu().numpy().view(np.uint32), (ov.cpu().numpy().view(np.uint32) if pairs else None)


def check(ls, torch, keys, offs, m, vals=None, inplace=False):
    gk, gv = run(ls, torch, keys, offs, m, vals, inplace)
    ek, ev = M.segments_expected(keys, [int(o) for o in offs], vals)
    M.assert_keys(gk, ek, f"m={m} inplace={inplace}")
    if vals is not None:
        np.testing.assert_array_equal(gv, ev)
    return gk, gv


def positions(n):
    return np.arange(n, dtype=np.uint32)


def tile(ls, pairs):
    return ls.segment_pair_tile_keys() if pairs else ls.segment_tile_keys()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("pairs", [False, True])
def test_every_short_length(ls, torch_gpu, pairs, inplace):
    offs = offsets_of(range(1, 131))
    n = int(offs[-1])
    keys = M.random_words((n,), 0xF5E0)
    keys[::5] = M.tie_words((n,), 0xF5E1)[::5]
    check(ls, torch_gpu, keys, offs, 130, positions(n) if pairs else None, inplace)


@pytest.mark.parametrize("pairs", [False, True])
def test_class_edges(ls, torch_gpu, pairs):
    edges = ls.segment_class_edges(pairs)
    T = edges[-1]
    lengths = []
    for E in edges[:-1]:
        lengths += [E - 1, 0, E, 1, E + 1]
    lengths += [T - 1, T]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = M.random_words((n,), 0xF5E2)
    keys[1::7] = M.normal_words((n,), 0xF5E3)[1::7]
    check(ls, torch_gpu, keys, offs, T, positions(n) if pairs else None)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("pairs", [False, True])
def test_full_segments_of_nans(ls, torch_gpu, pairs, inplace):
    """A NaN's image equals the padding sentinel: a full-capacity segment of every class that is all
    NaN, one with NaNs in its last slots, and partly filled ones beside them.  No key may be lost to
    the padding, and NaN payloads come out in position order."""
    edges = ls.segment_class_edges(pairs)
    T = edges[-1]
    rng = np.random.default_rng(0xF5E4)
    lengths, fills = [], []
    for E in [64] + list(edges):
        lengths += [E, E, E - 3, E]
        fills += ["all_nan", "nan_tail", "nan_tail", "nan_head"]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = M.random_words((n,), 0xF5E5)
    for (a, b), fill in zip(zip(offs[:-1], offs[1:]), fills):
        a, b = int(a), int(b)
        if fill == "all_nan":
            keys[a:b] = NAN_WORDS[rng.integers(0, NAN_WORDS.size, size=b - a)]
        elif fill == "nan_tail":
            keys[b - 40:b] = NAN_WORDS[rng.integers(0, NAN_WORDS.size, size=40)]
        else:
            keys[a:a + 40] = NAN_WORDS[rng.integers(0, NAN_WORDS.size, size=40)]
    vals = positions(n) if pairs else None
    gk, gv = check(ls, torch_gpu, keys, offs, T, vals, inplace)
    for (a, b), fill in zip(zip(offs[:-1], offs[1:]), fills):
        a, b = int(a), int(b)
        if fill == "all_nan":
            assert np.all(M.is_nan(gk[a:b]))
            if pairs:
                np.testing.assert_array_equal(gv[a:b], np.arange(a, b, dtype=np.uint32))


@pytest.mark.parametrize("path", ["lds", "general"])
def test_stability(ls, torch_gpu, path):
    e = ls.segment_class_edges(True)
    T = e[-1]
    lengths = list(range(0, 131, 7))
    for E in e[:-1]:
        lengths += [E - 1, E, E + 1]
    lengths += [T]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = M.tie_words((n,), 0xF5E6)
    check(ls, torch_gpu, keys, offs, T if path == "lds" else 0, positions(n))


@pytest.mark.parametrize("pairs", [False, True])
def test_many_tiny_segments(ls, torch_gpu, pairs):
    rng = np.random.default_rng(0xF5E7)
    lengths = rng.integers(0, 6, size=50_000)
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = M.random_words((n,), 0xF5E8)
    keys[::4] = M.tie_words((n,), 0xF5E9)[::4]
    check(ls, torch_gpu, keys, offs, 5, positions(n) if pairs else None)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("promise", [0, 40_000])
def test_general_path(ls, torch_gpu, promise, pairs, inplace):
    """max_segment_keys 0 (unknown) or past the tile: two pair sorts of the whole array, which take
    the key type through labsort_sort_pairs_device."""
    lengths = [17, 0, 40_000, 1, 300, 5000, 2, 64, 1025]
    offs = offsets_of(lengths)
    n = int(offs[-1])
    keys = M.random_words((n,), 0xF5EA)
    keys[17:17 + 40_000:3] = M.tie_words((40_000,), 0xF5EB)[::3]
    check(ls, torch_gpu, keys, offs, promise, positions(n) if pairs else None, inplace)


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("path", ["lds", "general"])
def test_rejected_offsets(ls, torch_gpu, path, pairs):
    torch = torch_gpu
    lengths = [10, 0, 300, 1, 64, 5000, 2, 100]
    good = offsets_of(lengths)
    n, nseg = int(good[-1]), len(lengths)
    m = 5000 if path == "lds" else 0
    offs = good.copy()
    offs[3] = offs[2] - 1  # decreases once
    keys = M.random_words((n,), 0xF5EC)
    vals = positions(n)
    dk, dv, do = dev(torch, keys), dev(torch, vals), dev(torch, offs)
    ok, ov = torch.full_like(dk, PATTERN), torch.full_like(dv, PATTERN)
    ws = ff_ws(ls, torch, n, nseg, m, pairs)

    def call(offsets):
        if pairs:
            ls.sort_segments_pairs_device(dk, dv, ok, ov, n, offsets, nseg, m, key="f32", workspace=ws)
        else:
            ls.sort_segments_device(dk, ok, n, offsets, nseg, m, key="f32", workspace=ws)

    call(do)
    with pytest.raises(ls.LabsortError) as ei:
        ls.segments_workspace_status(ws)
    assert ei.value.status == ls.ERR_ARG
    assert bool((ok == PATTERN).all())
    if pairs:
        assert bool((ov == PATTERN).all())
    call(dev(torch, good))  # a valid call on the same workspace afterwards succeeds
    ls.segments_workspace_status(ws)
    ek, ev = M.segments_expected(keys, [int(o) for o in good], vals if pairs else None)
    M.assert_keys(ok.cpu().numpy().view(np.uint32), ek)
    if pairs:
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), ev)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("pairs", [False, True])
def test_digit_masks(ls, torch_gpu, pairs, inplace):
    """The pass-skip logic of every class kernel: segments of 1 to 9000 keys and of the tile's length,
    each length once per set of differing digits (16 masks) and per variant of
    sort_sweep_model.digit_mask_rows (digits random per key, two values one bit apart, all keys equal
    but the first, the last or one in the middle; at the tile's length three of the five).  The
    payloads are the positions, so equal keys must keep their order whichever passes ran."""
    T = tile(ls, pairs)
    keys, offs, labels = S.mask_segments("f32", T, 0xF5F0)
    n = keys.size
    assert n < 4_000_000 and max(length for length, _, _ in labels) == T
    gk, gv = run(ls, torch_gpu, keys, offs, T, positions(n) if pairs else None, inplace)
    ek, ev = M.segments_expected(keys, [int(o) for o in offs], positions(n) if pairs else None)
    wrong = gk != ek  # (no NaN among these keys)
    if pairs:
        wrong |= gv != ev
    if wrong.any():
        s = int(np.searchsorted(offs.astype(np.int64), int(np.flatnonzero(wrong)[0]), side="right")) - 1
        raise AssertionError(f"pairs={pairs} inplace={inplace}: {int(wrong.sum())} elements differ, the first in segment {s}: "
                             f"{labels[s][0]} keys, mask {labels[s][1]:#x} {labels[s][2]}")
    M.assert_keys(gk, ek, f"pairs={pairs} inplace={inplace}")


@pytest.mark.parametrize("seed", S.F32SEG_SEEDS)
def test_seeded_sweep(ls, torch_gpu, seed):
    """60 cases per seed (sort_sweep_model.f32_segment_sweep_cases): up to 2^17 keys cut at random places,
    empty segments among them, few long segments in every third case; max_segment_keys the true
    maximum or 0 (both paths); keys or pairs with random payloads; in place or out of place; every
    segment from its own generator (digit masks, heavy ties with NaNs, NaNs only, sorted ...)."""
    cases = list(S.f32_segment_sweep_cases(seed, ls.segment_tile_keys(), ls.segment_pair_tile_keys()))
    failures, hit = [], {}
    for i, c in enumerate(cases):
        what = f"{c['path']} {'pairs' if c['pairs'] else 'keys'}"
        hit[what] = hit.get(what, 0) + 1
        try:
            check(ls, torch_gpu, c["keys"], c["offs"], c["m"], c["vals"], c["inplace"])
        except AssertionError as err:
            failures.append(f"seed {seed} case {i}: {c['tag']}: {str(err).strip().splitlines()[0]}")
    print(f"seed {seed}: {dict(sorted(hit.items()))}")
    assert not failures, failures


def _graph_lengths(rng, n, nseg, T):
    lengths = [int(rng.integers(4097, T + 1)) for _ in range(3)] + [int(rng.integers(257, 4097)) for _ in range(20)]
    while sum(lengths) < n:
        lengths.append(min(int(rng.integers(0, 257)), n - sum(lengths)))
    assert sum(lengths) == n and len(lengths) <= nseg
    lengths += [0] * (nseg - len(lengths))
    return rng.permutation(np.asarray(lengths))


@pytest.mark.parametrize("path", ["lds", "general"])
@pytest.mark.parametrize("pairs", [False, True])
def test_graph_replay(ls, torch_gpu, pairs, path):
    """One captured call replayed on new keys and new offsets in the same buffers."""
    torch = torch_gpu
    n, nseg = 200_000, 2048
    T = tile(ls, pairs)
    m = T if path == "lds" else 0
    src = torch.empty(n, dtype=torch.float32, device="cuda")
    vsrc = torch.empty(n, dtype=torch.int32, device="cuda")
    out, vout = torch.empty_like(src), torch.empty_like(vsrc)
    offs = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    ws = ff_ws(ls, torch, n, nseg, m, pairs)

    def load(seed):
        r = np.random.default_rng(seed)
        o = offsets_of(_graph_lengths(r, n, nseg, T))
        k = M.tie_words((n,), seed) if seed & 1 else M.random_words((n,), seed)
        v = r.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        src.view(torch.int32).copy_(dev(torch, k))
        vsrc.copy_(dev(torch, v))
        offs.copy_(dev(torch, o))
        return k, v, o

    def call(stream):
        if pairs:
            ls.sort_segments_pairs_device(src, vsrc, out, vout, n, offs, nseg, m, key="f32", workspace=ws, stream=stream)
        else:
            ls.sort_segments_device(src, out, n, offs, nseg, m, key="f32", workspace=ws, stream=stream)

    load(0xF5ED)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        call(s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream())
    for seed in (0xF5EE, 0xF5EF):
        k, v, o = load(seed)
        out.view(torch.int32).fill_(PATTERN)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.segments_workspace_status(ws)
        ek, ev = M.segments_expected(k, [int(x) for x in o], v if pairs else None)
        M.assert_keys(out.view(torch.int32).cpu().numpy().view(np.uint32), ek)
        if pairs:
            np.testing.assert_array_equal(vout.cpu().numpy().view(np.uint32), ev)
