"""The hybrid radix sort's finish since k_fin_block hands its list out by ticket and k_plan8 clears
only the look-back regions that will be read (csrc/fin_block.h, k_plan8).  Every
case runs under LABSORT_RADIX_HYBRID=2, asserts the path labsort_radix_path reports and compares
the result bit for bit with numpy's sort.

k_fin_block's list holds the buckets of 1025 to 5120 keys (shorter ones stay with the wave classes:
binning them into the block class was measured and not kept), so the inputs that must put an exact
number of entries on the ticketed list are made of its shortest buckets, 1025 to 1027 keys, and
carry two buckets of 20000 keys beside them, which are on the tile class's list: with a single
listed bucket the input would otherwise be below the 32769 keys from which the path is offered."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSIC, HYBRID = 0, 1
MODES = ("lean", "full", "auto")
# every length at which k_fin_block's stripes change shape, both ends of its class, then the tile class
BLOCK_LENS = (1, 2, 63, 64, 65, 255, 256, 257, 1024, 5119, 5120)
TILE_LENS = (5121, 20480)
FILLER = {0x0004: 20000, 0xFFF8: 20000}  # tile class, one top-14-bit group each


@pytest.fixture(autouse=True)
def hybrid_env(monkeypatch):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")


def rng(seed):
    return np.random.default_rng(0x71C4E700 + seed)


def buckets(r, sizes):
    """Shuffled uint32 keys: sizes[b] keys with top 16 bits b (a dict), random low 16 bits."""
    parts = [(np.uint32(b) << np.uint32(16)) | r.integers(0, 1 << 16, size=c, dtype=np.uint32) for b, c in sizes.items()]
    a = np.concatenate(parts)
    r.shuffle(a)
    return a


def expected(a, key):
    if key == "u32":
        return np.sort(a)
    view = np.int32 if key == "i32" else np.float32
    return np.sort(a.view(view)).view(np.uint32)


def sort_on(ls, torch, a, ws, key="u32", inplace=False, offset=0):
    """Sort the uint32 words a on the device with the workspace ws; (result, path, input afterwards)."""
    n = a.size
    src = torch.empty(n + offset, dtype=torch.int32, device="cuda")[offset:]
    src.copy_(torch.from_numpy(a.view(np.int32).copy()))
    out = src if inplace else torch.full((n + offset,), -7, dtype=torch.int32, device="cuda")[offset:]
    ls.sort_device(src.data_ptr(), out.data_ptr(), n, key=key, algo="radix", workspace=ws)
    ls.workspace_status(ws, n, "radix")
    return out.cpu().numpy().view(np.uint32), ls.radix_path(ws, n), src.cpu().numpy().view(np.uint32)


def workspace(ls, torch, n):
    return torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")


def check(ls, torch, a, want=HYBRID, ws=None, key="u32", **kw):
    assert a.size >= 32769
    got, path, src = sort_on(ls, torch, a, workspace(ls, torch, a.size) if ws is None else ws, key=key, **kw)
    assert path == want
    np.testing.assert_array_equal(got, expected(a, key))
    if not kw.get("inplace"):
        np.testing.assert_array_equal(src, a)


def short_buckets(r, count):
    """`count` buckets of 1025 to 1027 keys, one per top-14-bit group outside the filler's, and the filler."""
    free = np.array([b for b in range(1 << 14) if all(b != f >> 2 for f in FILLER)])
    ids = r.choice(free, size=count, replace=False) * 4 + r.integers(0, 4, size=count)
    sizes = {int(b): int(c) for b, c in zip(ids, r.integers(1025, 1028, size=count))}
    sizes.update(FILLER)
    return sizes


def grid(torch):
    return 5 * torch.cuda.get_device_properties(0).multi_processor_count


# the list's length against the grid g: no draw at all; the last first entry; exactly the grid; one
# ticket; one ticket in the third round; the last entry one short of a full round
EDGES = {"1": lambda g: 1, "g-1": lambda g: g - 1, "g": lambda g: g, "g+1": lambda g: g + 1, "2g+1": lambda g: 2 * g + 1,
         "3g-1": lambda g: 3 * g - 1}


@pytest.mark.parametrize("edge", list(EDGES))
def test_ticket_edges(ls, torch_gpu, edge):
    count = EDGES[edge](grid(torch_gpu))
    r = rng(list(EDGES).index(edge))
    sizes = short_buckets(r, count)
    assert sum(1 for c in sizes.values() if 1025 <= c <= 5120) == count
    check(ls, torch_gpu, buckets(r, sizes))


def test_every_bucket_short(ls, torch_gpu):
    """All 65536 buckets hold 1 or 2 keys: nothing on the ticketed list, the first wave class's as long as a list gets."""
    r = rng(10)
    check(ls, torch_gpu, buckets(r, {b: int(c) for b, c in enumerate(r.integers(1, 3, size=1 << 16))}))


def lengths_input(r, ids):
    lens = BLOCK_LENS + TILE_LENS
    assert len(ids) == len(lens)
    return buckets(r, dict(zip(ids, lens)))


def own_group_ids(r, count):
    """`count` bucket ids, each in a top-14-bit group of its own."""
    return (r.choice(1 << 14, size=count, replace=False) * 4 + r.integers(0, 4, size=count)).tolist()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
def test_lengths_of_both_classes(ls, torch_gpu, inplace, offset):
    """Buckets of 1 to 5120 keys (the wave classes and both ends of the block class) and of 5121 and 20480
    keys (tile class) in one input; in place and out of place; pointers 16-byte aligned and 4 bytes past."""
    r = rng(20)
    check(ls, torch_gpu, lengths_input(r, own_group_ids(r, len(BLOCK_LENS + TILE_LENS))), inplace=inplace, offset=offset)


def test_int32_keys(ls, torch_gpu):
    r = rng(21)
    ids = [0x7FFC, 0x7FF8, 0x0000, 0x0004, 0x8000, 0x8004, 0xFFFC, 0xFFF8, 0x4000, 0xC000, 0x2000, 0xA000, 0x6000]
    a = lengths_input(r, ids)
    assert (a.view(np.int32) < 0).any() and (a.view(np.int32) > 0).any()
    check(ls, torch_gpu, a, key="i32")


def test_float32_keys(ls, torch_gpu):
    """(no NaN and no zero among the keys: their words have one order)"""
    r = rng(22)
    ids = [0x3F80, 0x3F84, 0x0080, 0x7F00, 0xBF80, 0xBF84, 0x8080, 0xFF00, 0x4000, 0xC000, 0x2000, 0xA000, 0x6000]
    check(ls, torch_gpu, lengths_input(r, ids), key="f32")


def sized(r, sizes, n, pad_id):
    """sizes topped up to n keys by buckets of up to 20000 keys, one per top-14-bit group from pad_id on."""
    sizes, rest = dict(sizes), n - sum(sizes.values())
    assert rest >= 0 and pad_id % 4 == 0
    while rest:
        assert all(b >> 2 != pad_id >> 2 for b in sizes)
        sizes[pad_id] = min(rest, 20000)
        rest -= sizes[pad_id]
        pad_id += 4
    return buckets(r, sizes)


def classic_input(r, n):
    """One bucket of 40000 keys (too long for the path) among buckets of 100."""
    sizes = {int(b) + 4: 100 for b in r.choice((1 << 15) - 4, size=(n - 40000) // 100, replace=False)}
    sizes[0xC0DE] = n - 100 * len(sizes)
    assert sizes[0xC0DE] >= 40000
    return buckets(r, sizes)


@pytest.mark.parametrize("mode", MODES)
def test_workspace_reused_without_clearing(ls, torch_gpu, monkeypatch, mode):
    """Three different inputs of one size through one workspace, nothing cleared between the calls: ticketed
    lists of about 2 g, about 34 and about g entries, so a ticket or a look-back word left by the call before would show.
    Under every counting mode, so both of k_plan8's clear routes run."""
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    g, r = grid(torch_gpu), rng(30 + MODES.index(mode))
    n = (2 * g + 5) * 1027 + 60000
    ws = workspace(ls, torch_gpu, n)

    def outside_pad(sizes):  # (sized() pads from bucket 0x8000 on: at most n / 20000 + 1 groups)
        return {b: c for b, c in sizes.items() if not 0x8000 <= b < 0x8400}

    first = sized(r, outside_pad(short_buckets(r, 2 * g + 5)), n, 0x8000)
    long_lens = (1025, 2049, 3001, 4096, 4999, 5120)
    second = sized(r, {4 * i + 1: long_lens[i % len(long_lens)] for i in range(34)}, n, 0x8000)
    third = sized(r, outside_pad(short_buckets(r, g + 1)), n, 0x8000)
    for a in (first, second, third):
        assert a.size == n and n // 20000 + 1 <= 0x400 // 4
        check(ls, torch_gpu, a, ws=ws)


@pytest.mark.parametrize("mode", MODES)
def test_classic_after_hybrid_on_one_workspace(ls, torch_gpu, monkeypatch, mode):
    """classic, hybrid, classic: the second classic sort needs the look-back regions of digits 0 and 1, which
    the hybrid call between may have left as the first classic sort filled them."""
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    n, r = 1 << 18, rng(40 + MODES.index(mode))
    ws = workspace(ls, torch_gpu, n)
    check(ls, torch_gpu, classic_input(r, n), CLASSIC, ws=ws)
    check(ls, torch_gpu, r.integers(0, 1 << 32, size=n, dtype=np.uint32), HYBRID, ws=ws)
    check(ls, torch_gpu, classic_input(r, n), CLASSIC, ws=ws)


def test_graph_replay_hybrid_classic_hybrid(ls, torch_gpu):
    """One captured call replayed on a hybrid, a classic and a hybrid input (ticketed lists of g + 300 and
    g + 100 entries): the sequence zeroes its ticket itself and clears what the replay's path reads."""
    torch = torch_gpu
    n, r = 1 << 21, rng(50)
    assert (grid(torch) + 300) * 1027 + 40000 <= n
    eligible = [sized(r, {b: c for b, c in short_buckets(r, grid(torch) + extra).items() if not 0x8000 <= b < 0x8400}, n, 0x8000)
                for extra in (300, 100)]
    inputs = [(eligible[0], HYBRID), (classic_input(r, n), CLASSIC), (eligible[1], HYBRID)]
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(src)
    ws = workspace(ls, torch, n)
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
