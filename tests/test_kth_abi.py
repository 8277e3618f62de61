"""CPU tests of the k-th key selection's C ABI (labsort_kth_*, include/labsort.h): exports, the
host-side argument checks, the empty shapes, the workspace sizing, and ls.kthvalue's checks that come
before the device.  No kernel is launched: every call below returns before its first launch (the
pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import rowsort_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_kth_row_keys", "labsort_kth_workspace_bytes", "labsort_kth_device", "labsort_kth_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", R.KINDS)
# one launch (short rows, the edge of the path), the long path with whole and partial chunks
SHAPES = [(4, 100), (3, 4097), (2, 16384), (2, 16385), (2, 32768), (2, 70001)]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("kth_row_keys", "kth_workspace_bytes", "kth_device", "kth_workspace_status", "kthvalue"):
        assert callable(getattr(ls, f)), f
    assert hdr.index("labsort_sort16_device(") < hdr.index("labsort_kth_device(") < hdr.index("labsort_wave_tile_sort(")
    assert ls.kth_row_keys() == 16384  # TK_CHUNK: a row held by 1024 threads, 16 keys each


def test_kernel_classes_unchanged(ls):
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    assert "#define LABSORT_K_COUNT 11" in hdr
    assert len(ls.KCLASS) == 11 and ls.KCLASS["topk"] == 10


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in range(5):
        assert L.labsort_kth_device(None, 0, 10, 1, None, 0, kt, None, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_kth_device(None, 3, 0, 1, None, 1, kt, None, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_kth_device(None, 0, 0, 0, None, 0, kt, None, None, None, 0, None) == ls.OK
        assert L.labsort_kth_device(FAR + 1, 0, 10, 99, FAR + 2, 1, kt, FAR + 3, None, None, 0, None) == ls.OK
    assert L.labsort_kth_device(None, 0, 10, 1, None, 0, 9, None, None, None, 0, None) == ls.OK  # before the key type


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_argument_errors(ls, kind, rows, cols):
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    nin = rows * cols * esz  # bytes of the input
    nko, nw = rows * esz, rows * 4  # bytes of the key output; of the position output and of d_k
    need = ls.kth_workspace_bytes(rows, cols)
    for largest in (0, 1):
        def call(keys=FAR, out=2 * FAR, idx=3 * FAR, dk=None, k=1, ws=4 * FAR, wsb=BIG, r=rows, c=cols, kt=kt):
            return L.labsort_kth_device(keys, r, c, k, dk, largest, kt, out, idx, ws, wsb, None)
        assert call(keys=None) == ls.ERR_ARG and call(out=None) == ls.ERR_ARG
        for bad in (5, 7, -1):
            assert call(kt=bad) == ls.ERR_ARG
        # the host k counts only without d_k
        assert call(k=0) == ls.ERR_ARG and call(k=cols + 1) == ls.ERR_ARG and call(k=BIG) == ls.ERR_ARG
        assert call(r=0x7FFFFFFF // cols + 1) == ls.ERR_ARG  # rows * cols past 2^31 - 1
        assert call(idx=2 * FAR) == ls.ERR_ARG  # d_idx_out == d_keys_out
        # overlap by the real extents: on the input's last and first element, and the whole of it
        assert call(out=FAR + nin - esz) == ls.ERR_ARG
        assert call(out=FAR - nko + esz) == ls.ERR_ARG
        assert call(out=FAR) == ls.ERR_ARG
        assert call(idx=FAR + nin - 4) == ls.ERR_ARG
        assert call(idx=FAR - nw + 4) == ls.ERR_ARG
        assert call(idx=FAR) == ls.ERR_ARG
        # an output on d_k
        dk = 5 * FAR
        assert call(dk=dk, out=dk) == ls.ERR_ARG
        assert call(dk=dk, out=dk + nw - esz) == ls.ERR_ARG
        assert call(dk=dk, out=dk - nko + esz) == ls.ERR_ARG
        assert call(dk=dk, idx=dk) == ls.ERR_ARG
        assert call(dk=dk, idx=dk + nw - 4) == ls.ERR_ARG
        assert call(dk=dk, idx=dk - nw + 4) == ls.ERR_ARG
        # workspace: NULL, 16 bytes short, none; with and without positions, with and without d_k
        for idx in (3 * FAR, None):
            for dk_ in (None, dk):
                assert call(idx=idx, dk=dk_, ws=None, wsb=need) == ls.ERR_ARG
                assert call(idx=idx, dk=dk_, wsb=need - 16) == ls.ERR_ARG
                assert call(idx=idx, dk=dk_, wsb=0) == ls.ERR_ARG
        if esz == 2:  # odd addresses
            assert call(keys=FAR + 1) == ls.ERR_ARG and call(out=2 * FAR + 1) == ls.ERR_ARG
            assert call(keys=FAR + 1, out=2 * FAR + 1) == ls.ERR_ARG
        # Outputs directly behind and in front of the input and of d_k get past the overlap checks, and
        # with d_k a host k of 0 or past cols is ignored: these fail only on the (deliberately) NULL
        # workspace, the last thing looked at ...
        assert call(out=FAR + nin, idx=FAR - nw, ws=None) == ls.ERR_ARG
        assert call(dk=dk, out=dk + nw, idx=dk - nw, k=0, ws=None) == ls.ERR_ARG
        assert call(dk=dk, k=cols + 1, ws=None) == ls.ERR_ARG
    # ... which is the one thing wrong with them: each error above was reported with a good workspace


def test_rows_times_cols_limit(ls):
    L = ls.lib
    for kt in range(5):
        assert L.labsort_kth_device(FAR, 1 << 16, 1 << 15, 1, None, 0, kt, 2 * FAR, None, 3 * FAR, BIG, None) == ls.ERR_ARG
        assert L.labsort_kth_device(FAR, 1, 1 << 31, 1, None, 0, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG
        assert L.labsort_kth_device(FAR, 1 << 31, 1, 1, None, 1, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG


def test_workspace_size(ls):
    """The 256-byte header exactly up to kth_row_keys(); above it the histograms, the states and the
    count table: 1/16 byte per key and a little per row, far less than top-k's or the row sort's.
    Never shrinks over a grid of shapes."""
    Rk = ls.kth_row_keys()
    for rows in (1, 3, 1000, 1 << 17):
        for cols in (1, 2, 4097, Rk - 1, Rk):
            assert ls.kth_workspace_bytes(rows, cols) == 256
    assert ls.kth_workspace_bytes(0, 100000) == 256 and ls.kth_workspace_bytes(5, 0) == 256
    assert ls.kth_workspace_bytes(1, Rk + 1) > 256
    assert ls.kth_workspace_bytes(1, Rk + 1) > ls.kth_workspace_bytes(1 << 17, Rk)
    rows_grid = [1, 2, 3, 7, 64, 1000, 4096]
    cols_grid = [1, 100, Rk, Rk + 1, 2 * Rk, 2 * Rk + 1, 70001, 151936, 1 << 18, 1 << 19]
    for i, rows in enumerate(rows_grid):
        for j, cols in enumerate(cols_grid):
            w = ls.kth_workspace_bytes(rows, cols)
            assert w % 256 == 0
            if i:
                assert ls.kth_workspace_bytes(rows_grid[i - 1], cols) <= w
            if j:
                assert ls.kth_workspace_bytes(rows, cols_grid[j - 1]) <= w
            assert ls.kth_workspace_bytes(rows + 1, cols) >= w and ls.kth_workspace_bytes(rows, cols + 1) >= w
            if cols > Rk:
                chunks = -(-cols // Rk)
                assert w >= 256 + rows * chunks * 1024 + rows * 4096
                assert w <= 256 + rows * chunks * 1024 + rows * 4096 + rows * 256 + 3 * 256
                if rows * cols < 1 << 31:  # (a shape top-k takes)
                    assert w < ls.topk_workspace_bytes(rows, cols, 1)
    w = ls.kth_workspace_bytes(1, 1 << 28)
    assert (1 << 24) <= w <= (1 << 24) + (1 << 14)  # 2^28 keys in one row: 16 MiB of counts
    assert len(ls.lib.labsort_kth_workspace_bytes.argtypes) == 2  # no key type


def test_kthvalue_rejects_other_inputs_before_the_device(ls):
    """TypeError for a CPU tensor, a dtype that is no key type, a non-contiguous tensor and a k that is
    neither an int nor an int32 tensor, on CPU tensors, so before any device call."""
    import torch
    for dt in (torch.bfloat16, torch.float16, torch.float32, torch.int32):
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros((2, 40000), dtype=dt), 3)  # a CPU tensor
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros(100, dtype=dt), 3)
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros((40000, 2), dtype=dt).t(), 1)  # a transposed view
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros((2, 2, 100), dtype=dt), 1)
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros((2, 100), dtype=dt), torch.ones(2, dtype=torch.int32))  # (x on the CPU comes first)
    for dt in (torch.int64, torch.float64, torch.int16, torch.uint8):
        with pytest.raises(TypeError):
            ls.kthvalue(torch.zeros((2, 100), dtype=dt), 1)
    with pytest.raises(TypeError):
        ls.kthvalue(np.zeros((2, 100), dtype=np.float32), 1)
    doc = ls.kthvalue.__doc__
    assert "(cols + 1) // 2" in doc and "torch.median" in doc and "NaN" in doc
