"""k_fin_block, the block class (1025-5120 keys) of the hybrid radix sort's finish (DESIGN.md §3.9,
csrc/fin_block.h): two fixed LDS passes, a fold per wave, four workgroup barriers per bucket, none
between buckets, and the next bucket's keys loaded before this one's are stored.  Every case
asserts that the hybrid path ran (labsort_radix_path), compares the result bit for bit with
numpy.sort and, out of place, that the input is unchanged.  The inputs keep the path condition:
both low digits vary over the whole input, no top-14-bit group holds more than 32768 keys and
n >= 32769."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HYBRID = 1
# lengths at which the groups-per-wave count steps (a step every 256 keys) and the last wave's
# tail is 1, 63 or 64 keys; both ends of the class
BLOCK_LENS = (1025, 1279, 1280, 1281, 2048, 4095, 4096, 4097, 5119, 5120)
TILE_LEN = 5121  # the first length of the tile class


@pytest.fixture(autouse=True)
def hybrid_env(monkeypatch):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")


def rng(seed):
    return np.random.default_rng(0x5EEDF100 + seed)


def buckets(r, sizes):
    """Shuffled uint32 keys: sizes[b] keys with top 16 bits b (a dict), random low 16 bits."""
    parts = [(np.uint32(b) << np.uint32(16)) | r.integers(0, 1 << 16, size=c, dtype=np.uint32) for b, c in sizes.items()]
    a = np.concatenate(parts)
    r.shuffle(a)
    return a


def ordered_buckets(r, lows):
    """uint32 keys: bucket b holds the low halves lows[b] (a dict of arrays) in that order -- the
    scatter passes are stable, so this is the order the finish reads them in; the buckets follow
    one another in a random order."""
    ids = list(lows)
    r.shuffle(ids)
    return np.concatenate([(np.uint32(b) << np.uint32(16)) | lows[b].astype(np.uint32) for b in ids])


def run(ls, torch, a, key="u32", inplace=False, offset=0):
    """Sort the array a of 32-bit words on the device; (result, path, input afterwards)."""
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


def check(ls, torch, a, expect=None, **kw):
    assert a.size >= 32769
    got, path, src = run(ls, torch, a, **kw)
    assert path == HYBRID
    np.testing.assert_array_equal(got, np.sort(a) if expect is None else expect)
    if not kw.get("inplace"):
        np.testing.assert_array_equal(src, a)


def own_group_ids(r, count):
    """`count` bucket ids, each in a top-14-bit group of its own."""
    return (r.choice(1 << 14, size=count, replace=False) * 4 + r.integers(0, 4, size=count)).tolist()


def test_lengths_inside_the_block_class(ls, torch_gpu):
    """Every length of BLOCK_LENS and 5121, which the tile class sorts; one bucket per group."""
    r = rng(1)
    lens = list(BLOCK_LENS) + [TILE_LEN]
    check(ls, torch_gpu, buckets(r, dict(zip(own_group_ids(r, len(lens)), lens))))


def test_more_buckets_than_workgroups(ls, torch_gpu):
    """3000 block-class buckets of cycling lengths, ids four apart (8.8 M keys): 1280 workgroups
    sort two or three buckets of different lengths each, back to back with no barrier between."""
    r = rng(2)
    sizes = {4 * i: BLOCK_LENS[i % len(BLOCK_LENS)] for i in range(3000)}
    check(ls, torch_gpu, buckets(r, sizes))


def low_halves(r, kind, c):
    if kind == "equal":
        return np.full(c, r.integers(0, 1 << 16), dtype=np.uint32)
    if kind == "two_values":
        return r.choice(r.integers(0, 1 << 16, size=2, dtype=np.uint32), size=c)
    if kind == "digit0_uniform":
        return (r.integers(0, 256, size=c, dtype=np.uint32) << np.uint32(8)) | np.uint32(r.integers(0, 256))
    if kind == "digit1_uniform":
        return r.integers(0, 256, size=c, dtype=np.uint32) | np.uint32(int(r.integers(0, 256)) << 8)
    if kind == "all_ffff":
        return np.full(c, 0xFFFF, dtype=np.uint32)
    v = np.sort(r.integers(0, 1 << 16, size=c, dtype=np.uint32))
    return v if kind == "ascending" else v[::-1]


KINDS = ("equal", "two_values", "digit0_uniform", "digit1_uniform", "all_ffff", "ascending", "descending")


@pytest.mark.parametrize("kind", KINDS)
def test_low_halves(ls, torch_gpu, kind):
    """Buckets whose low halves stress the two fixed passes (lengths that are no multiple of 64
    among them: all_ffff is the padding's image), interleaved with ordinary buckets, which keep
    both low digits varying over the input; consecutive ids, so workgroups meet both sorts."""
    r = rng(10 + KINDS.index(kind))
    lens = (1025, 1343, 2049, 3001, 4096, 4999, 5120)
    lows = {}
    for i in range(42):
        c = lens[i % len(lens)]
        lows[4 * i] = low_halves(r, kind, c) if i % 2 == 0 else r.integers(0, 1 << 16, size=c, dtype=np.uint32)
    check(ls, torch_gpu, ordered_buckets(r, lows))


def test_int32_keys_on_both_sides_of_zero(ls, torch_gpu):
    r = rng(20)
    ids = [0x7FFC, 0x7FF8, 0x0000, 0x0004, 0x8000, 0x8004, 0xFFFC, 0xFFF8, 0x4000, 0xC000]
    ids += [i ^ 0x0100 for i in ids]
    a = buckets(r, dict(zip(ids, BLOCK_LENS * 2))).view(np.int32)
    assert (a < 0).any() and (a > 0).any()
    check(ls, torch_gpu, a, key="i32")


def test_float32_keys(ls, torch_gpu):
    """The whole-array float32 sort runs the uint32 sort on the order image, which keeps every
    bucket's length (no NaN and no zero among the keys: their words have one order)."""
    r = rng(21)
    ids = [0x3F80, 0x3F84, 0x0080, 0x7F00, 0xBF80, 0xBF84, 0x8080, 0xFF00, 0x4000, 0xC000]
    ids += [i ^ 0x0010 for i in ids]
    a = buckets(r, dict(zip(ids, BLOCK_LENS * 2)))
    expect = np.sort(a.view(np.float32)).view(np.uint32)
    check(ls, torch_gpu, a, expect=expect, key="f32")


@pytest.mark.parametrize("inplace", [False, True])
def test_keys_below_2_24(ls, torch_gpu, inplace):
    """One scatter pass (digit 2), 256 buckets of 1025-5120 keys; in place that pass lands in TMP
    and the finish reads TMP and writes OUT."""
    r = rng(22)
    sizes = {b: int(r.integers(1025, 5121)) for b in range(256)}
    sizes[7], sizes[100], sizes[255] = 1025, 5120, 4097
    check(ls, torch_gpu, buckets(r, sizes), inplace=inplace)


@pytest.mark.parametrize("inplace", [False, True])
def test_pointers_one_word_into_their_allocations(ls, torch_gpu, inplace):
    r = rng(23)
    sizes = {4 * i + 1: BLOCK_LENS[i % len(BLOCK_LENS)] for i in range(40)}
    check(ls, torch_gpu, buckets(r, sizes), inplace=inplace, offset=1)
