"""The hybrid radix finish's bucket offsets (k_fin_edges): bucket (d3, d2) starts where
the digit-3 pass put the first key of digit d3 at or after position S2[d2] of its input, read from that
pass's look-back region and one partial tile.  The cases place S2[d2], the number of keys with a smaller
digit 2, on and next to tile boundaries and segment starts (the digit-3 pass's segments are the 16
top nibbles of digit 2, its tiles 16384 keys aligned in the input but for a segment's first), at 0 and
at n, on runs of empty digit-2 values, and cover the plans with a constant digit 2 or digit 3.  Every
case asserts the hybrid path and compares bit for bit with numpy.sort.  Environment as in
test_gpu_radix_hybrid.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSIC, HYBRID = 0, 1
TILE = 16384


@pytest.fixture(autouse=True)
def hybrid_env(monkeypatch):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")


def rng(seed):
    return np.random.default_rng(0xF1ED6E00 + seed)


def counts_from_starts(fixed, n):
    """Keys per digit-2 value from chosen S2 values: fixed = {d2: S2[d2]}, S2[0] = 0 and S2[256] = n
    added, the values between two chosen ones spread evenly."""
    pts = {0: 0, 256: n, **fixed}
    d = sorted(pts)
    s2 = np.floor(np.interp(np.arange(257), d, [pts[i] for i in d])).astype(np.int64)
    for i in d:
        assert s2[i] == pts[i]
    c = np.diff(s2)
    assert (c >= 0).all() and c.sum() == n
    return c


def image_keys(r, counts, d3=(0, 256)):
    """Shuffled order images (key ^ flip): counts[d2] keys of digit 2 = d2, digit 3 uniform in
    [d3[0], d3[1]), random low 16 bits."""
    n = int(np.sum(counts))
    u = np.repeat(np.arange(256, dtype=np.uint32), counts) << np.uint32(16)
    u |= r.integers(d3[0], d3[1], size=n, dtype=np.uint32) << np.uint32(24)
    u |= r.integers(0, 1 << 16, size=n, dtype=np.uint32)
    r.shuffle(u)
    return u


def keys_of(u, key):
    """The keys of type `key` whose order images are u."""
    if key == "u32":
        return u
    if key == "i32":
        return (u ^ np.uint32(0x80000000)).view(np.int32)
    assert key == "f32"
    x = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
    assert np.isfinite(x).all() and (x != 0).all()  # numpy.sort's order is then the device's, bit for bit
    return x


def run(ls, torch, a, key="u32", inplace=False, offset=0):
    n = a.size
    host = torch.from_numpy(a.view(np.int32).copy())
    src = torch.empty(n + offset, dtype=torch.int32, device="cuda")[offset:]
    src.copy_(host)
    out = src if inplace else torch.full((n + offset,), -7, dtype=torch.int32, device="cuda")[offset:]
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    ls.sort_device(src.data_ptr(), out.data_ptr(), n, key=key, algo="radix", workspace=ws)
    ls.workspace_status(ws, n, "radix")
    return out.cpu().numpy().view(a.dtype), ls.radix_path(ws, n)


def check(ls, torch, a, **kw):
    got, path = run(ls, torch, a, **kw)
    assert path == HYBRID
    want = np.sort(a)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def tile_edge_counts():
    """n = 2^18.  S2 on a tile boundary that is a segment start (d2 = 16), one key before one (32: the
    segment's first tile has one key) and one key after (48); inside segment 4, which starts in the
    middle of a tile, on a boundary (70: the first tile's look-back word, nothing counted), one key
    after it (71) and one key before the next (79); a digit-2 value that fills one aligned tile (96)
    and the boundary right after it (97)."""
    n = 1 << 18
    fixed = {16: TILE, 32: 2 * TILE - 1, 48: 3 * TILE + 1, 64: 4 * TILE - 5000, 70: 4 * TILE, 71: 4 * TILE + 1,
             79: 5 * TILE - 1, 80: 5 * TILE, 96: 6 * TILE, 97: 7 * TILE, 98: 7 * TILE + 1}
    return counts_from_starts(fixed, n)


def sparse_counts(n):
    """Only digit-2 values 0, 16, 17, 31, 32 and 255 occur: S2 = 0 at d2 = 0 (and 1-16: no value
    between holds a key), long runs of equal S2, segment starts with keys (16, 32) and without (48,
    64, ...), an empty value right after a segment start (33); the values 33-255 all start where 255
    does, and the offsets of d2 = 255's ends are those of input position n."""
    c = np.zeros(256, dtype=np.int64)
    present = (0, 16, 17, 31, 32, 255)
    c[list(present)] = n // len(present)
    c[0] += n - c.sum()
    return c


def test_boundaries_on_tile_edges(ls, torch_gpu):
    check(ls, torch_gpu, image_keys(rng(1), tile_edge_counts()))


def test_segment_starts_and_empty_digit2_values(ls, torch_gpu):
    check(ls, torch_gpu, image_keys(rng(2), sparse_counts(1 << 18)))


def test_top_digit2_value_empty(ls, torch_gpu):
    """Nothing above digit-2 value 32: S2 = n for every value after it."""
    c = sparse_counts(1 << 18)
    c[32] += c[255]
    c[255] = 0
    check(ls, torch_gpu, image_keys(rng(3), c))


@pytest.mark.parametrize("n", [32769, 3 * TILE + 5])
def test_one_tile_plus_one_key_and_short_last_tile(ls, torch_gpu, n):
    check(ls, torch_gpu, rng(n).integers(0, 1 << 32, size=n, dtype=np.uint32))


def test_several_tiles_per_segment(ls, torch_gpu):
    """2^20 + 1 uniform keys: 64 tiles and more, a tile that is not its segment's first in every segment."""
    n = (1 << 20) + 1
    check(ls, torch_gpu, rng(4).integers(0, 1 << 32, size=n, dtype=np.uint32))


def test_digit2_values_inside_one_tile(ls, torch_gpu):
    """2^20 + 1 keys; digit-2 value 0x40 fills exactly one aligned tile, and the values 0x94-0x9B all
    lie inside one tile, which is not its segment's first: both ends of their buckets are counted
    in the same tile."""
    n = (1 << 20) + 1
    fixed = {0x40: 16 * TILE, 0x41: 17 * TILE, 0x80: 32 * TILE + 100, 0x90: 36 * TILE + 7, 0x94: 37 * TILE + 3,
             0x9C: 38 * TILE - 3}
    check(ls, torch_gpu, image_keys(rng(5), counts_from_starts(fixed, n)))


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("const", [0, 255])
@pytest.mark.parametrize("n", [3 * TILE + 5, 1 << 18])
def test_trivial_digit2(ls, torch_gpu, n, const, inplace):
    """Digit 2 constant: the digit-3 pass runs as one chain, S2 is 0 up to the constant and n above."""
    a = rng(6).integers(0, 1 << 32, size=n, dtype=np.uint32)
    check(ls, torch_gpu, (a & np.uint32(0xFF00FFFF)) | np.uint32(const << 16), inplace=inplace)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("const", [0, 255])
@pytest.mark.parametrize("n", [3 * TILE + 5, 1 << 18])
def test_trivial_digit3(ls, torch_gpu, n, const, inplace):
    """Digit 3 constant: no digit-3 pass, the offsets are S2 at the constant, 0 below it and n above."""
    a = rng(7).integers(0, 1 << 32, size=n, dtype=np.uint32)
    check(ls, torch_gpu, (a & np.uint32(0x00FFFFFF)) | np.uint32(const << 24), inplace=inplace)


def test_signed_keys(ls, torch_gpu):
    a = keys_of(image_keys(rng(8), tile_edge_counts()), "i32")
    assert (a < 0).any() and (a > 0).any()
    check(ls, torch_gpu, a, key="i32")


def test_float_keys(ls, torch_gpu):
    """float32 keys whose order images have the sparse digit-2 values (digit 3 in 1..254: finite)."""
    a = keys_of(image_keys(rng(9), sparse_counts(1 << 18), d3=(1, 255)), "f32")
    assert (a < 0).any() and (a > 0).any()
    check(ls, torch_gpu, a, key="f32")


@pytest.mark.parametrize("inplace", [False, True])
def test_unaligned_pointers(ls, torch_gpu, inplace):
    """Views one word into their allocations: the partial-tile reads start anywhere."""
    check(ls, torch_gpu, image_keys(rng(10), tile_edge_counts()), inplace=inplace, offset=1)


def test_graph_replay(ls, torch_gpu):
    """One captured call replayed over a hybrid input, a classic one (a 40000-key bucket) and a hybrid
    one again: the offsets come from the look-back region of the replay at hand."""
    torch = torch_gpu
    n = 1 << 18
    r = rng(11)
    classic = image_keys(r, sparse_counts(n))
    classic[:40000] = (classic[:40000] & np.uint32(0xFFFF)) | np.uint32(0xC0DE0000)
    inputs = [(image_keys(r, tile_edge_counts()), HYBRID), (classic, CLASSIC), (image_keys(r, sparse_counts(n)), HYBRID)]
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(src)
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    src.copy_(torch.from_numpy(inputs[0][0].view(np.int32)))
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
