"""Pins the edges of the upfront counts' uint4 loop as it stands (k_hist_lean in hist_lean.hip,
k_hist_seg in kernels.hip): groups of NU x HIST_BLOCK uint4, the next group loaded
while the current one is counted, a per-uint4 loop for what is left of the aligned body, scalar
loops for the head and the tail.  A pipelined form of that loop was built, measured and dropped;
these cases were written against it and now guard the loop that stayed.  They do not probe the
order of the lean count's flush and ticket: a missed count there would be a rare event that no
sort of this size shows (harness/exp/lean_count_probe.hip checks the last workgroup's sum).
The sizes put every workgroup's aligned body at k groups and one uint4 less or more, for
k = 1 .. 4: the last group counted without a successor, lanes that drop out of the last group
(-1) and the per-uint4 tail behind it (+1).  One size is shorter than a group, one is odd, with
scalar heads and tails, and one has two workgroups per position segment.  Each case sorts through
the public entry under LABSORT_HY_COUNT=lean and =full, asserts the path and the count that ran
and a clean workspace, and compares the result bit for bit with a CPU sort."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSIC, HYBRID = 0, 1
FULL_ONLY, LEAN_ONLY, LEAN_THEN_FULL = 0, 1, 2
NSEG, HIST_BLOCK, NU = 16, 1024, 4  # common.h; uint4 per thread and group in both counts
HS_MIN_KEYS, HS_BPS = 65536, 16
GROUP = NU * HIST_BLOCK  # uint4 per group


def parts_uint4(n, misaligned=False):
    """The uint4 count of every counting workgroup's aligned body (None: the scalar path), from
    seg_start's and the kernels' arithmetic."""
    if misaligned:
        return [None] * NSEG
    bps = min(max(n // (NSEG * HS_MIN_KEYS), 1), HS_BPS)
    out = []
    for seg in range(NSEG):
        sb, se = seg * n // NSEG, (seg + 1) * n // NSEG
        per = (se - sb + bps - 1) // bps
        for part in range(bps):
            beg = min(sb + part * per, se)
            end = min(beg + per, se)
            vbeg = min((beg + 3) & ~3, end)
            out.append((end - vbeg) // 4)
    return out


def exact(k, d):
    """n at which all 16 workgroups count exactly k groups and d uint4, no scalar head or tail."""
    return NSEG * 4 * (GROUP * k + d)


# name -> (n, the uint4 counts a workgroup's body may have)
SIZES = {f"k{k}{d:+d}": (exact(k, d), {GROUP * k + d}) for k in (1, 2, 3) for d in (-1, 0, 1)}
SIZES["k4+0"] = (exact(4, 0), {GROUP * 4})
SIZES["short"] = (NSEG * 4 * 1000, {1000})
SIZES["odd"] = (exact(2, 0) + 7, {GROUP * 2 - 1, GROUP * 2})
SIZES["two_parts"] = (1 << 21, {GROUP * 4})  # 32 workgroups
VARIANTS = ("u32", "unaligned", "i32", "f32", "digit0_constant", "one_group")


def test_sizes_produce_the_intended_parts():
    for name, (n, want) in SIZES.items():
        got = parts_uint4(n)
        assert n <= 1 << 21 and len(got) == (2 * NSEG if name == "two_parts" else NSEG), name
        assert set(got) <= want and want & set(got), (name, sorted(set(got)))
    n = SIZES["odd"][0]
    assert n % 2 == 1 and any((s * n // NSEG) % 4 for s in range(1, NSEG))  # scalar heads and tails
    assert SIZES["short"][0] // NSEG // 4 < GROUP


def image(a, key):
    """The uint32 order image of the key words a."""
    b = a.view(np.uint32)
    if key == "i32":
        return b ^ np.uint32(0x80000000)
    if key == "f32":
        return np.where(b >> np.uint32(31) != 0, ~b, b ^ np.uint32(0x80000000))
    return b


def rule(img):
    """k_plan8's rule at LABSORT_RADIX_HYBRID=2's bound: hybrid iff digits 0 and 1 both vary and no
    top-14-bit group holds more than 32768 keys."""
    diff = int(np.bitwise_and.reduce(img) ^ np.bitwise_or.reduce(img))
    top = np.bincount(img >> np.uint32(18), minlength=1 << 14).max()
    return HYBRID if (diff & 0xFF) and (diff & 0xFF00) and top <= 32768 else CLASSIC


def case(size, variant):
    """(key words as uint32, key type, expected words, expected path); both count modes share them."""
    n = SIZES[size][0]
    r = np.random.default_rng([0xC0917, sorted(SIZES).index(size), VARIANTS.index(variant)])
    a = r.integers(0, 1 << 32, size=n, dtype=np.uint32)
    key = variant if variant in ("i32", "f32") else "u32"
    if variant == "i32":
        assert (a.view(np.int32) < 0).any() and (a.view(np.int32) > 0).any()
    elif variant == "f32":  # finite floats of both signs: no exponent of 255
        a = np.where((a >> np.uint32(23)) & np.uint32(0xFF) == 0xFF, a & np.uint32(~(1 << 23) & 0xFFFFFFFF), a)
        assert np.isfinite(a.view(np.float32)).all()
    elif variant == "digit0_constant":
        a = (a & np.uint32(0xFFFFFF00)) | np.uint32(0x5A)
    elif variant == "one_group":  # every key in one top-14-bit group, in four buckets of the top 16 bits
        a = (a & np.uint32(0x0003FFFF)) | np.uint32(0xBEE40000)
    img = image(a, key)
    want = rule(img)
    assert want == (CLASSIC if variant in ("digit0_constant", "one_group") else HYBRID)
    expect = a[np.argsort(img, kind="stable")]
    a.setflags(write=False)
    expect.setflags(write=False)
    return a, key, expect, want


def run(ls, torch, a, key, offset):
    n = a.size
    src = torch.empty(n + 4 + offset, dtype=torch.int32, device="cuda")[offset:offset + n]
    src.copy_(torch.from_numpy(a.view(np.int32).copy()))
    out = torch.full((n + 4 + offset,), -7, dtype=torch.int32, device="cuda")[offset:offset + n]
    ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
    ls.sort_device(src.data_ptr(), out.data_ptr(), n, key=key, algo="radix", workspace=ws)
    ls.workspace_status(ws, n, "radix")
    return out.cpu().numpy().view(np.uint32), ls.radix_path(ws, n), ls.radix_counting(ws, n)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_count_pipeline(ls, torch_gpu, monkeypatch, size, variant):
    monkeypatch.setenv("LABSORT_RADIX_IMPL", "onesweep")
    monkeypatch.setenv("LABSORT_RADIX_HYBRID", "2")
    a, key, expect, want = case(size, variant)
    offset = 1 if variant == "unaligned" else 0  # a base one word off 16 bytes: the scalar path
    for mode in ("lean", "full"):
        monkeypatch.setenv("LABSORT_HY_COUNT", mode)
        got, path, counting = run(ls, torch_gpu, a, key, offset)
        assert (mode, path) == (mode, want)
        if mode == "full":
            assert counting == FULL_ONLY
        else:
            assert counting == (LEAN_ONLY if want == HYBRID else LEAN_THEN_FULL)
        np.testing.assert_array_equal(got, expect)
