"""CPU tests of the counting entries' C ABI (labsort_bucket_counts_*, labsort_bincount_*,
include/labsort.h): exports, every argument error the header lists for all eight key types, the key
types bincount refuses, the size limits, the workspace sizing, and the Python wrappers' checks that come
before the device.  No kernel is launched: every call below returns before its first launch (the
pointers are made-up addresses, far apart)."""
import os
import re
import subprocess

import pytest

import bucket_counts_model as BM
import searchsorted_model as SM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_bucket_counts_row_edges", "labsort_bucket_counts_workspace_bytes", "labsort_bucket_counts_device",
         "labsort_bincount_row_bins", "labsort_bincount_device"]
FAR = 1 << 40
BIG = 1 << 62
EDGES, VALUES, OUT, WS = 1 * FAR, 3 * FAR, 4 * FAR, 5 * FAR
ALL = pytest.mark.parametrize("kind", SM.KINDS)
BIN = pytest.mark.parametrize("kind", BM.BIN_KINDS)
LIM = (1 << 31) - 1


def call(ls, kind, nedges, rows=3, nv=100, edge_rows=None, right=0, edges=EDGES, values=VALUES, out=OUT, ws=WS, wsb=BIG, kt=None):
    edge_rows = rows if edge_rows is None else edge_rows
    return ls.lib.labsort_bucket_counts_device(edges, edge_rows, nedges, values, rows, nv, right,
                                               ls.KEY[kind] if kt is None else kt, out, ws, wsb, None)


def bcall(ls, kind, nbins, rows=3, nv=100, values=VALUES, out=OUT, kt=None):
    return ls.lib.labsort_bincount_device(values, rows, nv, nbins, ls.KEY[kind] if kt is None else kt, out, None)


def shapes(ls, kind):
    """(nedges, rows, nv, edge_rows) on both paths and in both forms."""
    E, V = ls.bucket_counts_row_edges(kind), ls.searchsorted_chunk_values()
    return [(c, r, nv, s) for c in (1, 100, E, E + 1, 3 * E + 5) for r, nv, s in ((1, 1, 1), (3, V + 1, 3), (3, 7, 1))]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    declared = set(re.findall(r"\b(labsort_(?:bucket_counts|bincount)_\w+)\s*\(", hdr))
    assert declared == set(NAMES) == {s for s in ls.C_SYMBOLS if s.startswith(("labsort_bucket_counts_", "labsort_bincount_"))}
    for f in ("bucket_counts_row_edges", "bucket_counts_workspace_bytes", "bucket_counts_device", "bincount_row_bins",
              "bincount_device", "bucket_counts", "bincount"):
        assert callable(getattr(ls, f)), f
    assert len(ls.lib.labsort_bucket_counts_device.argtypes) == 12
    assert len(ls.lib.labsort_bucket_counts_workspace_bytes.argtypes) == 3
    assert len(ls.lib.labsort_bincount_device.argtypes) == 7
    # the older digit count keeps its names
    assert "labsort_histogram" in ls.C_SYMBOLS and callable(ls.histogram)


def test_shapes_and_header_lists(ls):
    for kind in SM.KINDS:
        E, e = ls.bucket_counts_row_edges(kind), SM.esz(kind)
        # the sample table's 4096 strides start past the LDS path, and two workgroups' images and
        # counters fit a CU's 160 KB of LDS
        assert E >= SM.SAMPLES, kind
        assert 2 * (E * e + (E + 1) * 4) <= 160 * 1024, kind
        assert E <= ls.searchsorted_row_keys(kind)
    assert ls.bucket_counts_row_edges("f32") == ls.bucket_counts_row_edges("i32") == ls.bucket_counts_row_edges("u32")
    assert ls.bucket_counts_row_edges("f64") < ls.bucket_counts_row_edges("f32") < ls.bucket_counts_row_edges("bf16")
    for kt in (5, 6, 7, 11, -1):
        assert ls.lib.labsort_bucket_counts_row_edges(kt) == 0
    assert 256 <= ls.bincount_row_bins() and 2 * (ls.bincount_row_bins() + 1) * 4 <= 160 * 1024
    # the header's "accepted by ... only" lists of the float, 16-bit and 64-bit key types name the entry
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for define in ("#define LABSORT_KEY_F32 2", "#define LABSORT_KEY_BF16 3", "#define LABSORT_KEY_U64 8"):
        comment = hdr[:hdr.index(define)].rsplit("/*", 1)[1]
        assert "labsort_bucket_counts_device" in comment and "only" in comment.lower(), define
    assert "torch.bincount differs" in hdr


@ALL
def test_good_arguments_pass_the_checks(ls, kind):
    """With everything right but a NULL workspace a long-path call gets as far as the workspace check:
    the last one.  The error cases below each change one thing of a call that is otherwise good."""
    E = ls.bucket_counts_row_edges(kind)
    for nedges, rows, nv, s in shapes(ls, kind):
        if nedges > E:
            assert call(ls, kind, nedges, rows, nv, s, ws=None) == ls.ERR_ARG
            assert call(ls, kind, nedges, rows, 0, s, values=None, ws=None) == ls.ERR_ARG  # (nv == 0 does not skip it)


@ALL
def test_nothing_to_do_comes_first(ls, kind):
    """rows == 0: LABSORT_OK before anything else is looked at."""
    for nv in (0, 5):
        assert call(ls, kind, 100, 0, nv) == ls.OK
        assert call(ls, kind, 1 << 40, 0, nv, edge_rows=7, edges=None, values=None, out=None, ws=None, wsb=0, kt=77) == ls.OK
        assert call(ls, kind, 100, 0, nv, edges=EDGES + 1, values=VALUES + 1, out=OUT + 1) == ls.OK


def test_bincount_nothing_to_do_comes_first(ls):
    for kt in (0, 1, 8, 9, 2, 77):
        assert bcall(ls, "u32", 1 << 40, rows=0, nv=1 << 40, values=None, out=None, kt=kt) == ls.OK


@ALL
def test_null_pointers(ls, kind):
    for nedges, rows, nv, s in shapes(ls, kind):
        assert call(ls, kind, nedges, rows, nv, s, edges=None) == ls.ERR_ARG
        assert call(ls, kind, nedges, rows, nv, s, values=None) == ls.ERR_ARG
        assert call(ls, kind, nedges, rows, nv, s, out=None) == ls.ERR_ARG
    for s in (1, 3):  # nedges == 0 and nv == 0 still need an output; nedges == 0 still needs values
        assert call(ls, kind, 0, 3, 7, s, edges=None, values=None) == ls.ERR_ARG
        assert call(ls, kind, 0, 3, 7, s, edges=None, out=None) == ls.ERR_ARG
        assert call(ls, kind, 100, 3, 0, s, values=None, out=None) == ls.ERR_ARG
        assert call(ls, kind, 100, 3, 0, s, edges=None, values=None) == ls.ERR_ARG


def test_bad_key_types(ls):
    for kt in (5, 6, 7, 11, 12, -1, 1 << 20):
        for nedges in (0, 1, 100, 1 << 20):
            assert call(ls, "u32", nedges, kt=kt) == ls.ERR_ARG
            assert call(ls, "u32", nedges, 1, 1, 1, kt=kt) == ls.ERR_ARG
        assert ls.lib.labsort_bucket_counts_workspace_bytes(1, 1 << 20, kt) == 0
        assert bcall(ls, "u32", 100, kt=kt) == ls.ERR_ARG


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "f64"])
def test_bincount_refuses_the_non_integer_key_types(ls, kind):
    for nbins in (0, 1, 1000, ls.bincount_row_bins() + 1):
        for rows, nv in ((1, 1), (3, 100)):
            assert bcall(ls, kind, nbins, rows, nv) == ls.ERR_ARG


@ALL
def test_edge_rows_is_one_or_rows(ls, kind):
    for nedges in (0, 1, 100, ls.bucket_counts_row_edges(kind) + 1):
        for rows, s in ((3, 2), (3, 0), (3, 4), (1, 0), (1, 2), (257, 256)):
            assert call(ls, kind, nedges, rows, 9, s) == ls.ERR_ARG, (nedges, rows, s)


@ALL
def test_misaligned_pointers(ls, kind):
    e = SM.esz(kind)
    for nedges, rows, nv, s in shapes(ls, kind):
        for off in sorted({1, e // 2, e - 1} - {0}):
            assert call(ls, kind, nedges, rows, nv, s, edges=EDGES + off) == ls.ERR_ARG
            assert call(ls, kind, nedges, rows, nv, s, values=VALUES + off) == ls.ERR_ARG
        for off in (1, 2, 3):
            assert call(ls, kind, nedges, rows, nv, s, out=OUT + off) == ls.ERR_ARG
        if nedges > ls.bucket_counts_row_edges(kind):
            for off in (1, 4, 8):
                assert call(ls, kind, nedges, rows, nv, s, ws=WS + off) == ls.ERR_ARG


@BIN
def test_bincount_pointers(ls, kind):
    e = SM.esz(kind)
    for nbins in (1, 1000, ls.bincount_row_bins() + 1):
        for rows, nv in ((1, 1), (3, 4097)):
            assert bcall(ls, kind, nbins, rows, nv, values=None) == ls.ERR_ARG
            assert bcall(ls, kind, nbins, rows, nv, out=None) == ls.ERR_ARG
            assert bcall(ls, kind, nbins, rows, 0, values=None, out=None) == ls.ERR_ARG
            for off in sorted({1, e // 2, e - 1}):
                assert bcall(ls, kind, nbins, rows, nv, values=VALUES + off) == ls.ERR_ARG
            for off in (1, 2, 3):
                assert bcall(ls, kind, nbins, rows, nv, out=OUT + off) == ls.ERR_ARG
            ob = rows * (nbins + 1) * 4
            assert bcall(ls, kind, nbins, rows, nv, out=VALUES) == ls.ERR_ARG
            assert bcall(ls, kind, nbins, rows, nv, out=VALUES + rows * nv * e - 4) == ls.ERR_ARG
            assert bcall(ls, kind, nbins, rows, nv, out=VALUES - ob + 4) == ls.ERR_ARG


@ALL
def test_output_overlaps_an_input(ls, kind):
    """d_counts_out placed on the last element and, from below, on the first of each input and of the
    workspace, by the real extents."""
    e = SM.esz(kind)
    E = ls.bucket_counts_row_edges(kind)
    for nedges, rows, nv, s in shapes(ls, kind):
        ob = rows * (nedges + 1) * 4
        for base, ext in ((EDGES, s * nedges * e), (VALUES, rows * nv * e)):
            last = base + ext - min(e, 4)
            last -= last % 4
            assert call(ls, kind, nedges, rows, nv, s, out=last) == ls.ERR_ARG
            assert call(ls, kind, nedges, rows, nv, s, out=base - ob + 4) == ls.ERR_ARG
            assert call(ls, kind, nedges, rows, nv, s, out=base) == ls.ERR_ARG
        if nedges > E:
            need = ls.bucket_counts_workspace_bytes(s, nedges, kind)
            assert call(ls, kind, nedges, rows, nv, s, out=WS + need - 4) == ls.ERR_ARG
            assert call(ls, kind, nedges, rows, nv, s, out=WS - ob + 4) == ls.ERR_ARG


@ALL
def test_size_limits(ls, kind):
    assert call(ls, kind, 100, 1 << 16, 1 << 15, 1) == ls.ERR_ARG              # rows * nv = 2^31
    assert call(ls, kind, 100, 1, LIM + 1, 1) == ls.ERR_ARG
    assert call(ls, kind, 100, (1 << 32) + 1, 1 << 32, 1) == ls.ERR_ARG        # (a product that wraps)
    assert call(ls, kind, LIM + 1, 1, 5, 1) == ls.ERR_ARG                      # edge_rows * nedges = 2^31
    assert call(ls, kind, 1 << 16, 1 << 15, 5) == ls.ERR_ARG
    assert call(ls, kind, (1 << 32) + 3, 1 << 32, 1, 1 << 32) == ls.ERR_ARG
    assert call(ls, kind, LIM, 1, 5, 1) == ls.ERR_ARG                          # rows * (nedges + 1) = 2^31
    assert call(ls, kind, (1 << 15) - 1, 1 << 16, 5, 1) == ls.ERR_ARG          # the same with one shared edge row
    assert call(ls, kind, (1 << 64) - 1, 1, 5, 1) == ls.ERR_ARG                # (nedges + 1 wraps)
    assert call(ls, kind, (1 << 63) - 1, 2, 5, 1) == ls.ERR_ARG                # (rows * (nedges + 1) wraps)
    # at the limit the call goes on to the workspace check
    assert call(ls, kind, LIM - 1, 1, 5, 1, ws=None) == ls.ERR_ARG and call(ls, kind, LIM - 1, 1, 5, 1, wsb=4096) == ls.ERR_ARG


@BIN
def test_bincount_size_limits(ls, kind):
    assert bcall(ls, kind, 100, 1 << 16, 1 << 15) == ls.ERR_ARG
    assert bcall(ls, kind, 100, 1, LIM + 1) == ls.ERR_ARG
    assert bcall(ls, kind, 100, (1 << 32) + 1, 1 << 32) == ls.ERR_ARG
    assert bcall(ls, kind, LIM, 1, 5) == ls.ERR_ARG
    assert bcall(ls, kind, (1 << 15) - 1, 1 << 16, 5) == ls.ERR_ARG
    assert bcall(ls, kind, (1 << 64) - 1, 1, 5) == ls.ERR_ARG
    assert bcall(ls, kind, (1 << 63) - 1, 2, 5) == ls.ERR_ARG


@ALL
def test_workspace_errors(ls, kind):
    E = ls.bucket_counts_row_edges(kind)
    for nedges, rows, nv, s in shapes(ls, kind):
        need = ls.bucket_counts_workspace_bytes(s, nedges, kind)
        if nedges <= E:
            assert need == 0
            continue
        for wsb in (need - 1, need - 256, 256, 0):
            assert call(ls, kind, nedges, rows, nv, s, wsb=wsb) == ls.ERR_ARG
        assert call(ls, kind, nedges, rows, nv, s, ws=None, wsb=need) == ls.ERR_ARG


@ALL
def test_workspace_size(ls, kind):
    E, e = ls.bucket_counts_row_edges(kind), SM.esz(kind)
    for s in (1, 2, 3, 257, 1 << 16):
        for nedges in (0, 1, 64, E - 1, E):
            assert ls.bucket_counts_workspace_bytes(s, nedges, kind) == 0  # the LDS path: no workspace
        prev = 0
        for nedges in (E + 1, E + 2, 2 * E, 3 * E + 5, 1 << 20, 3 * (1 << 20) + 5, 1 << 28, LIM):
            w = ls.bucket_counts_workspace_bytes(s, nedges, kind)
            assert w >= prev and w % 256 == 0 and w >= 256 + s * SM.SAMPLES * e, (s, nedges)
            assert w <= 256 + s * (SM.SAMPLES * e + 256)  # a header and 8 to 32 KB per edge row, nothing per edge
            assert w == ls.searchsorted_workspace_bytes(s, max(nedges, ls.searchsorted_row_keys(kind) + 1), kind)
            prev = w
    for nedges in (E + 1, 1 << 24):
        prev = 0
        for s in (1, 2, 3, 4, 100, 257, 4096):
            w = ls.bucket_counts_workspace_bytes(s, nedges, kind)
            assert w > prev
            prev = w


def test_python_rejects_before_the_device(ls):
    import torch
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(TypeError, match="CUDA"):
        ls.bucket_counts(z(5), z(10))
    with pytest.raises(TypeError, match="CUDA"):
        ls.bucket_counts(z(5, torch.float32), z(10, torch.float32), right=True)
    with pytest.raises(TypeError, match="contiguous"):
        ls.bucket_counts(z(5), z(20)[::2])
    with pytest.raises(TypeError, match="contiguous"):
        ls.bucket_counts(z(10)[::2], z(20))
    with pytest.raises(TypeError, match="one dtype"):
        ls.bucket_counts(z(5, torch.float32), z(10))
    with pytest.raises(TypeError, match="one dtype"):
        ls.bucket_counts(z(5, torch.int64), z(10))
    for dt in (torch.int16, torch.int8, torch.bool):
        with pytest.raises(TypeError, match="expected, got"):
            ls.bucket_counts(z(5, dt), z(10, dt))
        with pytest.raises(TypeError, match="expected, got"):
            ls.bucket_counts(z(5, dt), z(10))
        with pytest.raises(TypeError, match="expected, got"):
            ls.bincount(z(5, dt), 10)
    with pytest.raises(TypeError, match="expected, got"):
        ls.bucket_counts(z(5), [1, 2, 3])
    with pytest.raises(TypeError, match="expected, got"):
        ls.bucket_counts(3, z(5))
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="expected, got"):
            ls.bincount(z(5, dt), 10)
    with pytest.raises(TypeError, match="expected, got"):
        ls.bincount([1, 2], 10)
    with pytest.raises(TypeError, match="CUDA"):
        ls.bincount(z(5), 10)
    with pytest.raises(TypeError, match="contiguous"):
        ls.bincount(z(10)[::2], 10)
    # (the shape checks come after the device check, as in searchsorted(): they are made on CUDA
    # tensors in tests/test_gpu_bucket_counts.py)
