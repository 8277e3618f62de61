"""The hybrid radix path's own upfront count (hist_lean.hip): two counters per key
and the AND / OR of the keys, the path's rule evaluated by the last workgroup to finish, the full
count as the fallback.  LABSORT_HY_COUNT chooses which count runs first (lean, full, or auto: a
sample of the keys decides); the path and the result never depend on it.  Every case compares the
result bit for bit with numpy.sort and asserts labsort_radix_path and labsort_radix_counting
(0 the full count only, 1 the lean count only, 2 the lean count and then the full one).
LABSORT_RADIX_HYBRID=2 opens the host gate at these sizes, with 32768 keys per top-14-bit group as
the rule's bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSIC, HYBRID = 0, 1
FULL_ONLY, LEAN_ONLY, LEAN_THEN_FULL = 0, 1, 2
SIZES = (32769, 3 * 16384 + 5, 1 << 18, (1 << 20) + 1)
MODES = ("lean", "full", "auto")
# labsort_workspace_bytes(n, LABSORT_ALGO_RADIX) of the build before the lean count existed
PARENT_WORKSPACE = {32769: 2031872, 3 * 16384 + 5: 2097408, 1 << 18: 3014656, (1 << 20) + 1: 9961472,
                    (1 << 21) + 777: 19005440}


@pytest.fixture(autouse=True)
def hybrid_env(monkeypatch):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")
    monkeypatch.delenv("LABSORT_HY_COUNT", raising=False)


def rng(seed):
    return np.random.default_rng(0x1EA2C000 + seed)


def uniform(seed, n):
    return rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint32)


def buckets(r, sizes):
    """Shuffled uint32 keys: sizes[b] keys with top 16 bits b (a dict), random low 16 bits."""
    parts = [(np.uint32(b) << np.uint32(16)) | r.integers(0, 1 << 16, size=c, dtype=np.uint32) for b, c in sizes.items()]
    a = np.concatenate(parts)
    r.shuffle(a)
    return a


def rule(a):
    """The path the device must choose for the uint32 order image a (k_plan8's rule at the gate's
    sound bound): hybrid iff digits 0 and 1 both vary and no top-14-bit group exceeds 32768 keys."""
    diff = int(np.bitwise_and.reduce(a) ^ np.bitwise_or.reduce(a))
    top = np.bincount(a >> np.uint32(18), minlength=1 << 14).max()
    return HYBRID if (diff & 0xFF) and (diff & 0xFF00) and top <= 32768 else CLASSIC


def sample_positions(n):
    """The predictor's sample (hist_lean.hip): 256 runs of 64 keys, one per 1/256th of the input."""
    r = np.arange(256, dtype=np.uint64)
    span = n // 256
    off = (((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)) % np.uint64(span - 63)
    return ((r * np.uint64(span) + off)[:, None] + np.arange(64, dtype=np.uint64)[None, :]).ravel()


def run(ls, torch, a, key="u32", inplace=False, offset=0):
    """Sort the uint32 / int32 array a on the device; (result, path, counting)."""
    n = a.size
    host = torch.from_numpy(a.view(np.int32).copy())
    src = torch.empty(n + offset, dtype=torch.int32, device="cuda")[offset:]
    src.copy_(host)
    out = src if inplace else torch.full((n + offset,), -7, dtype=torch.int32, device="cuda")[offset:]
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    ls.sort_device(src.data_ptr(), out.data_ptr(), n, key=key, algo="radix", workspace=ws)
    ls.workspace_status(ws, n, "radix")
    return out.cpu().numpy().view(a.dtype), ls.radix_path(ws, n), ls.radix_counting(ws, n)


def check(ls, torch, a, want_path, want_counting, **kw):
    """want_counting: a value, or a tuple of the admissible ones"""
    got, path, counting = run(ls, torch, a, **kw)
    assert path == want_path
    assert counting in (want_counting if isinstance(want_counting, tuple) else (want_counting,))
    np.testing.assert_array_equal(got, np.sort(a))


# the four inputs the rule rejects
def one_bucket_of_32769():
    r = rng(2)
    sizes = {int(b): 50 for b in r.choice(1 << 16, size=200, replace=False)}
    sizes[0x1234] = 32769
    return buckets(r, sizes)


def four_buckets_in_one_group():
    r = rng(3)
    sizes = {0x8000 + 4 * i: 300 for i in range(1, 40)}
    sizes.update({0x8000 + q: 10000 for q in range(4)})
    return buckets(r, sizes)


def constant_digit(digit):
    a = uniform(6 + digit, 1 << 18)
    return (a & np.uint32(0xFFFFFFFF ^ (0xFF << (8 * digit)))) | np.uint32(0x5A << (8 * digit))


REJECTED = {"bucket_32769": one_bucket_of_32769, "group_40000": four_buckets_in_one_group,
            "digit0_constant": lambda: constant_digit(0), "digit1_constant": lambda: constant_digit(1)}


@pytest.mark.parametrize("n", SIZES)
def test_uniform_in_every_mode(ls, torch_gpu, monkeypatch, n):
    a = uniform(n, n)
    results = []
    for mode, counting in zip(MODES, (LEAN_ONLY, FULL_ONLY, LEAN_ONLY)):
        monkeypatch.setenv("LABSORT_HY_COUNT", mode)
        got, path, c = run(ls, torch_gpu, a)
        assert (mode, path, c) == (mode, HYBRID, counting)
        results.append(got)
    np.testing.assert_array_equal(results[0], np.sort(a))
    np.testing.assert_array_equal(results[1], results[0])
    np.testing.assert_array_equal(results[2], results[0])


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_lean_falls_back_to_the_full_count(ls, torch_gpu, monkeypatch, name):
    a = REJECTED[name]()
    assert rule(a) == CLASSIC
    monkeypatch.setenv("LABSORT_HY_COUNT", "lean")
    check(ls, torch_gpu, a, CLASSIC, LEAN_THEN_FULL)


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_auto_on_rejected_inputs(ls, torch_gpu, name):
    """The sample may or may not see it coming: the full count runs either way."""
    check(ls, torch_gpu, REJECTED[name](), CLASSIC, (FULL_ONLY, LEAN_THEN_FULL))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("inplace", [False, True])
def test_trivial_digit3(ls, torch_gpu, monkeypatch, mode, inplace):
    """All keys below 2^24: digit 3 is constant, which the sums of four top14 counts show."""
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    a = rng(4).integers(0, 1 << 24, size=1 << 18, dtype=np.uint32)
    check(ls, torch_gpu, a, HYBRID, FULL_ONLY if mode == "full" else LEAN_ONLY, inplace=inplace)


@pytest.mark.parametrize("mode", MODES)
def test_trivial_digit2(ls, torch_gpu, monkeypatch, mode):
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    a = (uniform(5, 3 * 16384 + 5) & np.uint32(0xFF00FFFF)) | np.uint32(0x00A50000)
    check(ls, torch_gpu, a, HYBRID, FULL_ONLY if mode == "full" else LEAN_ONLY)


@pytest.mark.parametrize("mode", ["lean", "auto"])
@pytest.mark.parametrize("where", ["last", "outside_sample"])
def test_digit0_varies_in_one_key_only(ls, torch_gpu, monkeypatch, mode, where):
    """Digit 0 is 0x5A in every key but one: the rule says hybrid, and the lean count's AND / OR
    must have seen that key.  The sample sees a constant digit unless it holds the key."""
    n = 1 << 18
    a = (uniform(16, n) & np.uint32(0xFFFFFF00)) | np.uint32(0x5A)
    sample = set(sample_positions(n).tolist())
    pos = n - 1 if where == "last" else next(i for i in range(n // 2, n) if i not in sample)
    a[pos] ^= np.uint32(0x81)
    assert rule(a) == HYBRID
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    check(ls, torch_gpu, a, HYBRID, LEAN_ONLY if mode == "lean" or pos in sample else FULL_ONLY)


def test_sorted_keys(ls, torch_gpu, monkeypatch):
    """0..n-1: whole waves on one counter of either field (add_field's one add per wave)."""
    n = 1 << 18
    a = np.arange(n, dtype=np.uint32)
    assert rule(a) == CLASSIC  # one top-14-bit group holds them all
    monkeypatch.setenv("LABSORT_HY_COUNT", "lean")
    check(ls, torch_gpu, a, CLASSIC, LEAN_THEN_FULL)


def test_sorted_keys_spread_over_the_groups(ls, torch_gpu, monkeypatch):
    """i << 14: sorted, 16 keys per top-14-bit group, digits 0 and 1 vary: hybrid by the lean count."""
    n = 1 << 18
    a = np.arange(n, dtype=np.uint32) << np.uint32(14) | (np.arange(n, dtype=np.uint32) * np.uint32(40503) & np.uint32(0x3FFF))
    assert rule(a) == HYBRID
    monkeypatch.setenv("LABSORT_HY_COUNT", "lean")
    check(ls, torch_gpu, a, HYBRID, LEAN_ONLY)


@pytest.mark.parametrize("shuffled", [False, True])
def test_two_buckets(ls, torch_gpu, monkeypatch, shuffled):
    """Every key in one of two buckets of 32768 keys, in two top-14-bit groups: exactly the bound."""
    r = rng(17)
    a = buckets(r, {0x0421: 32768, 0xBEE5: 32768})
    if not shuffled:
        a = np.concatenate([a[a >> np.uint32(16) == 0xBEE5], a[a >> np.uint32(16) == 0x0421]])
    assert rule(a) == HYBRID
    monkeypatch.setenv("LABSORT_HY_COUNT", "lean")
    check(ls, torch_gpu, a, HYBRID, LEAN_ONLY)


@pytest.mark.parametrize("mode", ["lean", "auto"])
@pytest.mark.parametrize("inplace", [False, True])
def test_unaligned_pointers(ls, torch_gpu, monkeypatch, mode, inplace):
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    check(ls, torch_gpu, uniform(12, 1 << 18), HYBRID, LEAN_ONLY, inplace=inplace, offset=1)


@pytest.mark.parametrize("mode", ["lean", "auto"])
def test_signed_keys(ls, torch_gpu, monkeypatch, mode):
    a = rng(9).integers(-(1 << 31), 1 << 31, size=1 << 18, dtype=np.int64).astype(np.int32)
    assert (a < 0).any() and (a > 0).any()
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    check(ls, torch_gpu, a, HYBRID, LEAN_ONLY, key="i32")


def test_scalar_head_and_tail(ls, torch_gpu, monkeypatch):
    """Position segments that start and end off a 16-byte boundary."""
    n = (1 << 18) + 3
    assert any((s * n // 16) % 4 for s in range(1, 16))
    monkeypatch.setenv("LABSORT_HY_COUNT", "lean")
    check(ls, torch_gpu, uniform(18, n), HYBRID, LEAN_ONLY)


@pytest.mark.parametrize("mode", ["lean", "auto"])
def test_two_workgroups_per_segment(ls, torch_gpu, monkeypatch, mode):
    """2^21 + 777 keys: 32 counting workgroups, so the ticket counts past the 16 segments."""
    n = (1 << 21) + 777
    monkeypatch.setenv("LABSORT_HY_COUNT", mode)
    check(ls, torch_gpu, uniform(19, n), HYBRID, LEAN_ONLY)


def test_graph_replay_follows_the_data(ls, torch_gpu):
    """One captured call (auto) replayed on a hybrid, a classic and a hybrid input: path and counting
    follow the data; the sequence re-zeroes its ticket and verdict words itself."""
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
        counting = ls.radix_counting(ws, n)
        assert counting == LEAN_ONLY if want == HYBRID else counting != LEAN_ONLY
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), np.sort(a))


def test_workspace_size_unchanged(ls):
    for n, size in PARENT_WORKSPACE.items():
        assert ls.workspace_bytes(n, "radix") == size
