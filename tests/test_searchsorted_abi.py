"""CPU tests of the searchsorted entry's C ABI (labsort_searchsorted_*, include/labsort.h): exports,
every argument error the header lists for all eight key types, the workspace sizing, and the Python
wrappers' checks that come before the device.  No kernel is launched: every call below returns before
its first launch (the pointers are made-up addresses, far apart)."""
import os
import re
import subprocess

import pytest

import searchsorted_model as SM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_searchsorted_row_keys", "labsort_searchsorted_chunk_values", "labsort_searchsorted_workspace_bytes",
         "labsort_searchsorted_device"]
FAR = 1 << 40
BIG = 1 << 62
SORTED, SORTER, VALUES, OUT, WS = 1 * FAR, 2 * FAR, 3 * FAR, 4 * FAR, 5 * FAR
ALL = pytest.mark.parametrize("kind", SM.KINDS)
LIM = (1 << 31) - 1


def call(ls, kind, cols, rows=3, nv=100, seq_rows=None, right=0, sorted_=SORTED, sorter=None, values=VALUES, out=OUT, ws=WS,
         wsb=BIG, kt=None):
    seq_rows = rows if seq_rows is None else seq_rows
    return ls.lib.labsort_searchsorted_device(sorted_, seq_rows, cols, sorter, values, rows, nv, right,
                                              ls.KEY[kind] if kt is None else kt, out, ws, wsb, None)


def shapes(ls, kind):
    """(cols, rows, nv, seq_rows) on both paths and in both forms."""
    L, V = ls.searchsorted_row_keys(kind), ls.searchsorted_chunk_values()
    return [(c, r, nv, s) for c in (1, 100, L, L + 1, 3 * L + 5) for r, nv, s in ((1, 1, 1), (3, V + 1, 3), (3, 7, 1))]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    declared = set(re.findall(r"\b(labsort_searchsorted_\w+)\s*\(", hdr))
    assert declared == set(NAMES) == {s for s in ls.C_SYMBOLS if s.startswith("labsort_searchsorted_")}
    for f in ("searchsorted_row_keys", "searchsorted_chunk_values", "searchsorted_workspace_bytes", "searchsorted_device",
              "searchsorted", "bucketize"):
        assert callable(getattr(ls, f)), f
    assert len(ls.lib.labsort_searchsorted_device.argtypes) == 13
    assert len(ls.lib.labsort_searchsorted_workspace_bytes.argtypes) == 3


def test_shapes_and_header_lists(ls):
    V = ls.searchsorted_chunk_values()
    assert 512 <= V <= 65536 and V % 64 == 0
    for kind in SM.KINDS:
        L = ls.searchsorted_row_keys(kind)
        # at least two workgroups' images fit a CU's 160 KB of LDS, and a sample table fits one
        assert SM.SAMPLES <= L and 2 * L * SM.esz(kind) <= 160 * 1024, kind
    assert ls.searchsorted_row_keys("f32") == 2 * ls.searchsorted_row_keys("f64") == ls.searchsorted_row_keys("f16") // 2
    for kt in (5, 6, 7, 11, -1):
        assert ls.lib.labsort_searchsorted_row_keys(kt) == 0
    # the header's "accepted by ... only" lists of the float, 16-bit and 64-bit key types name the entry
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for define in ("#define LABSORT_KEY_F32 2", "#define LABSORT_KEY_BF16 3", "#define LABSORT_KEY_U64 8"):
        comment = hdr[:hdr.index(define)].rsplit("/*", 1)[1]
        assert "labsort_searchsorted_device" in comment and "only" in comment.lower(), define
    assert "torch.searchsorted differs" in hdr


@ALL
def test_good_arguments_pass_the_checks(ls, kind):
    """With everything right but a NULL workspace a long-path call gets as far as the workspace check:
    the last one.  The error cases below each change one thing of a call that is otherwise good."""
    L = ls.searchsorted_row_keys(kind)
    for cols, rows, nv, s in shapes(ls, kind):
        for sorter in (None, SORTER):
            if cols > L:
                assert call(ls, kind, cols, rows, nv, s, sorter=sorter, ws=None) == ls.ERR_ARG


@ALL
def test_nothing_to_do_comes_first(ls, kind):
    """rows == 0 or nv == 0: LABSORT_OK before anything else is looked at."""
    for rows, nv in ((0, 5), (5, 0), (0, 0)):
        assert call(ls, kind, 100, rows, nv) == ls.OK
        assert call(ls, kind, 1 << 40, rows, nv, seq_rows=7, sorted_=None, values=None, out=None, ws=None, wsb=0, kt=77) == ls.OK


@ALL
def test_null_pointers(ls, kind):
    for cols, rows, nv, s in shapes(ls, kind):
        assert call(ls, kind, cols, rows, nv, s, sorted_=None) == ls.ERR_ARG
        assert call(ls, kind, cols, rows, nv, s, values=None) == ls.ERR_ARG
        assert call(ls, kind, cols, rows, nv, s, out=None) == ls.ERR_ARG
    for s in (1, 3):  # cols == 0 still needs values and an output
        assert call(ls, kind, 0, 3, 7, s, sorted_=None, values=None) == ls.ERR_ARG
        assert call(ls, kind, 0, 3, 7, s, sorted_=None, out=None) == ls.ERR_ARG


def test_bad_key_types(ls):
    for kt in (5, 6, 7, 11, 12, -1, 1 << 20):
        for cols in (0, 1, 100, 1 << 20):
            assert call(ls, "u32", cols, kt=kt) == ls.ERR_ARG
            assert call(ls, "u32", cols, 1, 1, 1, kt=kt) == ls.ERR_ARG
        assert ls.lib.labsort_searchsorted_workspace_bytes(1, 1 << 20, kt) == 0


@ALL
def test_seq_rows_is_one_or_rows(ls, kind):
    for cols in (1, 100, ls.searchsorted_row_keys(kind) + 1):
        for rows, s in ((3, 2), (3, 0), (3, 4), (1, 0), (1, 2), (257, 256)):
            assert call(ls, kind, cols, rows, 9, s) == ls.ERR_ARG, (cols, rows, s)


@ALL
def test_misaligned_pointers(ls, kind):
    e = SM.esz(kind)
    for cols, rows, nv, s in shapes(ls, kind):
        for off in sorted({1, e // 2, e - 1} - {0}):
            assert call(ls, kind, cols, rows, nv, s, sorted_=SORTED + off) == ls.ERR_ARG
            assert call(ls, kind, cols, rows, nv, s, values=VALUES + off) == ls.ERR_ARG
        for off in (1, 2, 3):
            assert call(ls, kind, cols, rows, nv, s, out=OUT + off) == ls.ERR_ARG
            assert call(ls, kind, cols, rows, nv, s, sorter=SORTER + off) == ls.ERR_ARG
        if cols > ls.searchsorted_row_keys(kind):
            for off in (1, 4, 8):
                assert call(ls, kind, cols, rows, nv, s, ws=WS + off) == ls.ERR_ARG


@ALL
def test_output_overlaps_an_input(ls, kind):
    """d_out placed on the last element and, from below, on the first of each input and of the
    workspace, by the real extents."""
    e = SM.esz(kind)
    L = ls.searchsorted_row_keys(kind)
    for cols, rows, nv, s in shapes(ls, kind):
        ob = rows * nv * 4
        for base, ext, kw in ((SORTED, s * cols * e, {}), (VALUES, rows * nv * e, {}), (SORTER, s * cols * 4, dict(sorter=SORTER))):
            last = base + ext - min(e, 4)
            last -= last % 4
            assert call(ls, kind, cols, rows, nv, s, out=last, **kw) == ls.ERR_ARG
            assert call(ls, kind, cols, rows, nv, s, out=base - ob + 4, **kw) == ls.ERR_ARG
            assert call(ls, kind, cols, rows, nv, s, out=base, **kw) == ls.ERR_ARG
        if cols > L:
            need = ls.searchsorted_workspace_bytes(s, cols, kind)
            assert call(ls, kind, cols, rows, nv, s, out=WS + need - 4) == ls.ERR_ARG
            assert call(ls, kind, cols, rows, nv, s, out=WS - ob + 4) == ls.ERR_ARG


@ALL
def test_size_limits(ls, kind):
    assert call(ls, kind, 100, 1 << 16, 1 << 15, 1) == ls.ERR_ARG              # rows * nv = 2^31
    assert call(ls, kind, 100, 1, LIM + 1, 1) == ls.ERR_ARG
    assert call(ls, kind, 100, (1 << 32) + 1, 1 << 32, 1) == ls.ERR_ARG        # (a product that wraps)
    assert call(ls, kind, LIM + 1, 1, 5, 1) == ls.ERR_ARG                      # seq_rows * cols = 2^31
    assert call(ls, kind, 1 << 16, 1 << 15, 5) == ls.ERR_ARG
    assert call(ls, kind, (1 << 32) + 3, 1 << 32, 1, 1 << 32) == ls.ERR_ARG
    # at the limit the call goes on to the workspace check
    assert call(ls, kind, LIM, 1, 5, 1, ws=None) == ls.ERR_ARG and call(ls, kind, LIM, 1, 5, 1, wsb=4096) == ls.ERR_ARG


@ALL
def test_workspace_errors(ls, kind):
    L = ls.searchsorted_row_keys(kind)
    for cols, rows, nv, s in shapes(ls, kind):
        need = ls.searchsorted_workspace_bytes(s, cols, kind)
        if cols <= L:
            assert need == 0
            continue
        for wsb in (need - 1, need - 256, 256, 0):
            assert call(ls, kind, cols, rows, nv, s, wsb=wsb) == ls.ERR_ARG
        assert call(ls, kind, cols, rows, nv, s, ws=None, wsb=need) == ls.ERR_ARG


@ALL
def test_workspace_size(ls, kind):
    L, e = ls.searchsorted_row_keys(kind), SM.esz(kind)
    for s in (1, 2, 3, 257, 1 << 16):
        for cols in (0, 1, 64, L - 1, L):
            assert ls.searchsorted_workspace_bytes(s, cols, kind) == 0  # the LDS path: no workspace
        prev = 0
        for cols in (L + 1, L + 2, 2 * L, 3 * L + 5, 1 << 20, 3 * (1 << 20) + 5, 1 << 28, LIM):
            w = ls.searchsorted_workspace_bytes(s, cols, kind)
            assert w >= prev and w % 256 == 0 and w >= 256 + s * SM.SAMPLES * e, (s, cols)
            assert w <= 256 + s * (SM.SAMPLES * e + 256)  # a header and 16 to 32 KB per sequence, nothing per key
            prev = w
    for cols in (L + 1, 1 << 24):
        prev = 0
        for s in (1, 2, 3, 4, 100, 257, 4096):
            w = ls.searchsorted_workspace_bytes(s, cols, kind)
            assert w > prev
            prev = w


def test_python_rejects_before_the_device(ls):
    import torch
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(TypeError, match="CUDA"):
        ls.searchsorted(z(10), z(5))
    with pytest.raises(TypeError, match="CUDA"):
        ls.bucketize(z(5, torch.float32), z(10, torch.float32))
    with pytest.raises(TypeError, match="contiguous"):
        ls.searchsorted(z(20)[::2], z(5))
    with pytest.raises(TypeError, match="contiguous"):
        ls.searchsorted(z(20), z(10)[::2])
    with pytest.raises(TypeError, match="one dtype"):
        ls.searchsorted(z(10), z(5, torch.float32))
    with pytest.raises(TypeError, match="one dtype"):
        ls.bucketize(z(5, torch.int64), z(10))
    for dt in (torch.int16, torch.int8, torch.bool):
        with pytest.raises(TypeError, match="expected, got"):
            ls.searchsorted(z(10, dt), z(5, dt))
        with pytest.raises(TypeError, match="expected, got"):
            ls.searchsorted(z(10), z(5, dt))
    with pytest.raises(TypeError, match="expected, got"):
        ls.searchsorted([1, 2, 3], z(5))
    with pytest.raises(TypeError, match="expected, got"):
        ls.bucketize(3, z(5))
    with pytest.raises(ValueError, match="contradicts"):
        ls.searchsorted(z(10), z(5), right=True, side="left")
    with pytest.raises(ValueError, match="side"):
        ls.searchsorted(z(10), z(5), side="middle")
    with pytest.raises(TypeError, match="sorter"):
        ls.searchsorted(z(10), z(5), sorter=z(10, torch.int64))
    with pytest.raises(TypeError, match="sorter"):
        ls.searchsorted(z(10), z(5), sorter=z(20)[::2])
    with pytest.raises(TypeError, match="CUDA"):
        ls.searchsorted(z(10), z(5), side="right", right=True, sorter=z(10))  # (side and right agree: the device check is next)
    with pytest.raises(ValueError, match="1-D"):
        ls.bucketize(z(5), torch.zeros((2, 5), dtype=torch.int32))
