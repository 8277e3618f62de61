"""The hybrid path of LABSORT_ALGO_RADIX for keys only: scatter passes on digits
2 and 3, then every bucket of the top 16 bits sorted in LDS.  The path is chosen on the device
(both low digits vary and no value of the top 14 bits has more than 32768 keys), so every case
asserts, with labsort_radix_path, which path it ran, and compares the result bit for bit with
numpy.sort.  LABSORT_RADIX_HYBRID=2 opens the host gate at these small sizes; the radix passes
start above one tile (32768 keys)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSIC, HYBRID = 0, 1
# upper length bounds of the finish's classes (segsort.h: the wave classes, HY_BLOCK_KEYS, the
# tile), and the segmented sort's own block edge, which the finish does not use
FINISH_EDGES = (256, 512, 1024, 5120, 32768)
SEG_BLOCK_EDGE = 4096
SIZES = (32769, 3 * 16384 + 5, 1 << 18, (1 << 20) + 1)


@pytest.fixture(autouse=True)
def hybrid_env(monkeypatch):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")


def rng(seed):
    return np.random.default_rng(0x5EEDB000 + seed)


def buckets(r, sizes):
    """Shuffled uint32 keys: sizes[b] keys with top 16 bits b (a dict), random low 16 bits."""
    parts = [(np.uint32(b) << np.uint32(16)) | r.integers(0, 1 << 16, size=c, dtype=np.uint32) for b, c in sizes.items()]
    a = np.concatenate(parts)
    r.shuffle(a)
    return a


def run(ls, torch, a, key="u32", inplace=False, offset=0):
    """Sort the uint32 / int32 array a on the device; (result, path, input afterwards)."""
    n = a.size
    host = torch.from_numpy(a.view(np.int32).copy())
    src = torch.empty(n + offset, dtype=torch.int32, device="cuda")[offset:]
    src.copy_(host)
    out = src if inplace else torch.full((n + offset,), -7, dtype=torch.int32, device="cuda")[offset:]
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    ls.sort_device(src.data_ptr(), out.data_ptr(), n, key=key, algo="radix", workspace=ws)
    ls.workspace_status(ws, n, "radix")
    path = ls.radix_path(ws, n)
    return out.cpu().numpy().view(a.dtype), path, src.cpu().numpy().view(a.dtype)


def check(ls, torch, a, want_path, **kw):
    got, path, _ = run(ls, torch, a, **kw)
    assert path == want_path
    np.testing.assert_array_equal(got, np.sort(a))


@pytest.mark.parametrize("n", SIZES)
def test_uniform(ls, torch_gpu, n):
    """Uniform keys: at 2^20 + 1 buckets of ~16 keys, most of the 65536 present, some with one key;
    at the smaller sizes most buckets are empty."""
    check(ls, torch_gpu, rng(n).integers(0, 1 << 32, size=n, dtype=np.uint32), HYBRID)


def test_engineered_bucket_sizes(ls, torch_gpu):
    """Buckets of 1, 2, 64, 65 keys, every class edge e and e + 1, and exactly 32768 keys, each in
    a top-14-bit group of its own (bucket ids four apart), so the bound holds."""
    lens = [1, 2, 64, 65, SEG_BLOCK_EDGE, SEG_BLOCK_EDGE + 1, 32768]
    for e in FINISH_EDGES[:-1]:
        lens += [e, e + 1]
    r = rng(1)
    ids = r.choice(1 << 14, size=len(lens), replace=False) * 4 + r.integers(0, 4, size=len(lens))
    check(ls, torch_gpu, buckets(r, dict(zip(ids.tolist(), lens))), HYBRID)


def test_bucket_of_32769_takes_classic(ls, torch_gpu):
    r = rng(2)
    sizes = {int(b): 50 for b in r.choice(1 << 16, size=200, replace=False)}
    sizes[0x1234] = 32769
    check(ls, torch_gpu, buckets(r, sizes), CLASSIC)


def test_conservative_bound_takes_classic(ls, torch_gpu):
    """Four buckets of 10000 keys that share their top 14 bits: each would fit, but the decision
    bounds a bucket by its top-14-bit group (40000 keys), so the classic passes run."""
    r = rng(3)
    sizes = {0x8000 + 4 * i: 300 for i in range(1, 40)}
    sizes.update({0x8000 + q: 10000 for q in range(4)})
    check(ls, torch_gpu, buckets(r, sizes), CLASSIC)


@pytest.mark.parametrize("inplace", [False, True])
def test_trivial_digit3(ls, torch_gpu, inplace):
    """All keys below 2^24: one scatter pass (digit 2), 256 buckets of ~1024 keys."""
    n = 1 << 18
    check(ls, torch_gpu, rng(4).integers(0, 1 << 24, size=n, dtype=np.uint32), HYBRID, inplace=inplace)


def test_trivial_digit2(ls, torch_gpu):
    """Digit 2 constant, digit 3 varies: one scatter pass (digit 3)."""
    n = 3 * 16384 + 5
    a = rng(5).integers(0, 1 << 32, size=n, dtype=np.uint32)
    check(ls, torch_gpu, (a & np.uint32(0xFF00FFFF)) | np.uint32(0x00A50000), HYBRID)


@pytest.mark.parametrize("digit", [0, 1])
def test_trivial_low_digit_takes_classic(ls, torch_gpu, digit):
    n = 1 << 18
    a = rng(6 + digit).integers(0, 1 << 32, size=n, dtype=np.uint32)
    mask = np.uint32(0xFFFFFFFF ^ (0xFF << (8 * digit)))
    check(ls, torch_gpu, (a & mask) | np.uint32(0x5A << (8 * digit)), CLASSIC)


def test_equal_low_bits_inside_every_bucket(ls, torch_gpu):
    """The low 16 bits are a function of the bucket: the finish finds nothing to reorder."""
    n = 1 << 18
    b = rng(8).integers(0, 1 << 16, size=n, dtype=np.uint32)
    check(ls, torch_gpu, (b << np.uint32(16)) | ((b * np.uint32(40503)) & np.uint32(0xFFFF)), HYBRID)


def test_signed_keys(ls, torch_gpu):
    n = 1 << 18
    a = rng(9).integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)
    assert (a < 0).any() and (a > 0).any()
    check(ls, torch_gpu, a, HYBRID, key="i32")


def test_in_place(ls, torch_gpu):
    n = (1 << 20) + 1
    check(ls, torch_gpu, rng(10).integers(0, 1 << 32, size=n, dtype=np.uint32), HYBRID, inplace=True)


def test_out_of_place_leaves_input(ls, torch_gpu):
    n = 3 * 16384 + 5
    a = rng(11).integers(0, 1 << 32, size=n, dtype=np.uint32)
    got, path, src = run(ls, torch_gpu, a)
    assert path == HYBRID
    np.testing.assert_array_equal(got, np.sort(a))
    np.testing.assert_array_equal(src, a)


@pytest.mark.parametrize("inplace", [False, True])
def test_unaligned_pointers(ls, torch_gpu, inplace):
    """Input and output views one word into their allocations (not 16-byte aligned)."""
    n = 1 << 18
    check(ls, torch_gpu, rng(12).integers(0, 1 << 32, size=n, dtype=np.uint32), HYBRID, inplace=inplace, offset=1)


def test_graph_replay_follows_the_data(ls, torch_gpu):
    """One captured sort_device call replayed on an eligible input, on one with a 40000-key bucket
    and on an eligible one again: the launch sequence is fixed, the path is chosen per replay."""
    torch = torch_gpu
    n = 1 << 18
    r = rng(13)
    eligible = [r.integers(0, 1 << 32, size=n, dtype=np.uint32) for _ in range(2)]
    sizes = {int(b): 100 for b in r.choice(1 << 15, size=(n - 40000) // 100, replace=False)}
    sizes[0xC0DE] = n - 100 * len(sizes)
    assert sizes[0xC0DE] >= 40000
    inputs = [(eligible[0], HYBRID), (buckets(r, sizes), CLASSIC), (eligible[1], HYBRID)]
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(src)
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    src.copy_(torch.from_numpy(eligible[0].view(np.int32)))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # warm-up outside the capture
        ls.sort_device(src, out, n, algo="radix", workspace=ws, stream=s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ls.sort_device(src, out, n, algo="radix", workspace=ws, stream=torch.cuda.current_stream())
    for a, want in inputs:
        src.copy_(torch.from_numpy(a.view(np.int32)))
        out.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ls.workspace_status(ws, n, "radix")
        assert ls.radix_path(ws, n) == want
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), np.sort(a))


def test_knob_off(ls, torch_gpu, monkeypatch):
    n = 1 << 18
    a = rng(14).integers(0, 1 << 32, size=n, dtype=np.uint32)
    on, path_on, _ = run(ls, torch_gpu, a)
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "0")
    off, path_off, _ = run(ls, torch_gpu, a)
    assert (path_on, path_off) == (HYBRID, CLASSIC)
    np.testing.assert_array_equal(off, np.sort(a))
    np.testing.assert_array_equal(on, off)


def test_default_gate_keeps_small_sorts_classic(ls, torch_gpu, monkeypatch):
    """Unset, the knob offers the hybrid path around 2^28 keys only."""
    monkeypatch.delenv("LABSORT_RADIX_HYBRID")
    n = 1 << 18
    check(ls, torch_gpu, rng(15).integers(0, 1 << 32, size=n, dtype=np.uint32), CLASSIC)
