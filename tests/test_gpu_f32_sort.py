"""labsort_sort_device / labsort_sort_pairs_device with float32 keys on the GPU, against the numpy model
of the contract (tests/f32_model.py: the stable argsort of ord(key)), at sizes that reach the
one-tile, gathered, onesweep and merge paths, with every algorithm, in place and out of place.
Keys compare NaN-ness everywhere and bit-exact otherwise, payloads exactly.  Every call runs on a
workspace filled with 0xFF and outputs filled with a pattern, is followed by the status call, and an
out-of-place call must leave its input as it was."""
import functools

import numpy as np
import pytest

import f32_model as M

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
SIZES = [1, 5, 32768, 32769, 40000, (1 << 16) + 3, (1 << 20) + 1]
ALGOS = ["radix", "merge", "auto"]


@functools.lru_cache(maxsize=None)
def case(n):
    """Keys (random words with the specials planted, a stretch of heavy ties, NaNs and zeros), the
    payloads (positions) and the expected outputs; computed once per size and never written."""
    keys = M.random_words((n,), 0xF500 + n % 1000)
    keys[n // 3:n // 3 + n // 4] = M.tie_words((n // 4,), 0xF501)
    if n >= 5:
        keys[-1] = 0x80000000  # -0.0 behind a +0.0 planted before it
        keys[0] = 0x00000000
    vals = np.arange(n, dtype=np.uint32)
    ek, ev = M.sort_expected(keys, vals)
    for a in (keys, vals, ek, ev):
        a.setflags(write=False)
    return keys, vals, ek, ev


def dev(torch, a):
    return torch.from_numpy(np.array(a).view(np.int32)).cuda()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", SIZES)
def test_sort_device(ls, torch_gpu, n, algo, inplace):
    torch = torch_gpu
    keys, _, ek, _ = case(n)
    d = dev(torch, keys)
    before = d.clone()
    out = d if inplace else torch.full_like(d, PATTERN)
    ws = torch.full((max(ls.workspace_bytes(n, algo), 256),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sort_device(d.view(torch.float32), out.view(torch.float32), n, key="f32", algo=algo, workspace=ws)
    ls.workspace_status(ws, n, algo)
    if not inplace:
        assert torch.equal(d, before), "the input was written"
    M.assert_keys(out.cpu().numpy().view(np.uint32), ek, f"n={n} {algo} inplace={inplace}")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", SIZES)
def test_sort_pairs_device(ls, torch_gpu, n, algo, inplace):
    """Stable: payload = position, with ties, NaNs of several payloads and both zeros among the keys."""
    torch = torch_gpu
    keys, vals, ek, ev = case(n)
    dk, dv = dev(torch, keys), dev(torch, vals)
    bk, bv = dk.clone(), dv.clone()
    ok = dk if inplace else torch.full_like(dk, PATTERN)
    ov = dv if inplace else torch.full_like(dv, PATTERN)
    ws = torch.full((max(ls.pairs_workspace_bytes(n, algo), 256),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sort_pairs_device(dk.view(torch.float32), dv, ok.view(torch.float32), ov, n, key="f32", algo=algo, workspace=ws)
    ls.pairs_workspace_status(ws, n, algo)
    if not inplace:
        assert torch.equal(dk, bk) and torch.equal(dv, bv), "the input was written"
    M.assert_keys(ok.cpu().numpy().view(np.uint32), ek, f"n={n} {algo} inplace={inplace}")
    np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), ev)


@pytest.mark.parametrize("pairs", [False, True])
def test_graph_replay(ls, torch_gpu, pairs):
    """One captured out-of-place call replayed on new keys in the same buffers."""
    torch = torch_gpu
    n, algo = (1 << 18) + 5, "auto"
    src = torch.zeros(n, dtype=torch.float32, device="cuda")
    vsrc = torch.arange(n, dtype=torch.int32, device="cuda")
    out, vout = torch.empty_like(src), torch.empty_like(vsrc)
    nbytes = ls.pairs_workspace_bytes(n, algo) if pairs else ls.workspace_bytes(n, algo)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")

    def call(stream):
        if pairs:
            ls.sort_pairs_device(src, vsrc, out, vout, n, key="f32", algo=algo, workspace=ws, stream=stream)
        else:
            ls.sort_device(src, out, n, key="f32", algo=algo, workspace=ws, stream=stream)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up outside the capture
        call(s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream())
    inputs = [M.normal_words((n,), 0xF502), M.tie_words((n,), 0xF503), M.random_words((n,), 0xF504)]
    for i, x in enumerate(inputs):
        src.view(torch.int32).copy_(dev(torch, x))
        out.view(torch.int32).fill_(PATTERN)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if pairs:
            ls.pairs_workspace_status(ws, n, algo)
        else:
            ls.workspace_status(ws, n, algo)
        ek, ev = M.sort_expected(x, np.arange(n, dtype=np.uint32))
        assert np.array_equal(src.view(torch.int32).cpu().numpy().view(np.uint32), x), "the input was written"
        M.assert_keys(out.view(torch.int32).cpu().numpy().view(np.uint32), ek, f"replay {i}")
        if pairs:
            np.testing.assert_array_equal(vout.cpu().numpy().view(np.uint32), ev)
