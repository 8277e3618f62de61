"""CPU tests of the top-k filter's C ABI (labsort_topk_mask_*, include/labsort.h): exports, the
host-side argument checks, the one alias allowed, the empty shapes, the workspace sizing, and the
checks of ls.topk_filter / ls.topk_mask that come before the device.  No kernel is launched: every call
below returns before its first launch (the pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import rowsort_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_topk_mask_workspace_bytes", "labsort_topk_mask_device", "labsort_topk_mask_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", R.KINDS)
SHAPES = [(4, 100), (3, 4097), (2, 16384), (2, 16385), (2, 70001)]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("topk_mask_workspace_bytes", "topk_mask_device", "topk_mask_workspace_status", "topk_filter", "topk_mask"):
        assert callable(getattr(ls, f)), f
    assert hdr.index("labsort_kth_device(") < hdr.index("labsort_topk_mask_device(") < hdr.index("labsort_unique_device(")
    assert len(ls.lib.labsort_topk_mask_device.argtypes) == 13


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in range(5):
        assert L.labsort_topk_mask_device(None, 0, 10, 1, None, 0, kt, 0, None, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_topk_mask_device(None, 3, 0, 1, None, 1, kt, 0, None, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_topk_mask_device(FAR + 1, 0, 10, 99, FAR + 2, 1, kt, 0xFFFFFFFF, FAR + 3, None, None, 0, None) == ls.OK
    assert L.labsort_topk_mask_device(None, 0, 10, 1, None, 0, 9, 0, None, None, None, 0, None) == ls.OK  # before the key type


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_argument_errors(ls, kind, rows, cols):
    """Each call changes one thing of a good one (call()'s defaults: far-apart buffers, k = 1, a
    workspace that is large enough), so each ERR_ARG comes from the one check that the change meets.
    The workspace is the last thing looked at: the calls that differ only in it are otherwise good."""
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    nin, nm, nw = rows * cols * esz, rows * cols, rows * 4  # bytes of the keys, of the mask, of d_k
    need = ls.topk_mask_workspace_bytes(rows, cols)
    dk = 5 * FAR
    for largest in (0, 1):
        def call(keys=FAR, out=2 * FAR, mask=3 * FAR, dk=None, k=1, ws=4 * FAR, wsb=BIG, r=rows, c=cols, kt=kt, fill=0):
            return L.labsort_topk_mask_device(keys, r, c, k, dk, largest, kt, fill, out, mask, ws, wsb, None)
        assert call(keys=None) == ls.ERR_ARG
        assert call(out=None, mask=None) == ls.ERR_ARG
        for bad in (5, 6, 7, 8, 9, 10, 11, -1):  # 8 .. 10: the 64-bit types
            assert call(kt=bad) == ls.ERR_ARG
        assert call(k=0) == ls.ERR_ARG and call(k=cols + 1) == ls.ERR_ARG and call(k=BIG) == ls.ERR_ARG
        assert call(r=0x7FFFFFFF // cols + 1) == ls.ERR_ARG
        # keys output against the input: one element off the exact alias either way, on its last element, behind its first
        assert call(out=FAR + esz) == ls.ERR_ARG and call(out=FAR - esz) == ls.ERR_ARG
        assert call(out=FAR + nin - esz) == ls.ERR_ARG and call(out=FAR - nin + esz) == ls.ERR_ARG
        # the mask against the input and against the keys output (also in place)
        for base in (FAR, 2 * FAR):
            assert call(mask=base) == ls.ERR_ARG
            assert call(mask=base + nin - 1) == ls.ERR_ARG
            assert call(mask=base - nm + 1) == ls.ERR_ARG
        assert call(out=FAR, mask=FAR + nin - 1) == ls.ERR_ARG
        assert call(out=None, mask=FAR + 1) == ls.ERR_ARG
        # d_k against both outputs and the input
        for base, size in ((2 * FAR, nin), (3 * FAR, nm), (FAR, nin)):
            assert call(dk=base) == ls.ERR_ARG
            assert call(dk=base + size - 1) == ls.ERR_ARG
            assert call(dk=base - nw + 1) == ls.ERR_ARG
        assert call(out=FAR, dk=FAR + 4) == ls.ERR_ARG
        # workspace: NULL, 16 bytes short, none
        for out, mask in ((2 * FAR, 3 * FAR), (2 * FAR, None), (None, 3 * FAR), (FAR, None)):
            for dk_ in (None, dk):
                assert call(out=out, mask=mask, dk=dk_, ws=None, wsb=need) == ls.ERR_ARG
                assert call(out=out, mask=mask, dk=dk_, wsb=need - 16) == ls.ERR_ARG
                assert call(out=out, mask=mask, dk=dk_, wsb=0) == ls.ERR_ARG
        if esz == 2:
            assert call(keys=FAR + 1) == ls.ERR_ARG and call(out=2 * FAR + 1) == ls.ERR_ARG
            assert call(keys=FAR + 1, out=FAR + 1) == ls.ERR_ARG  # (the alias, but odd)
            for fill in (0x10000, 0xFFFF0000, 0x80000000, 0xFFFFFFFF):
                assert call(fill=fill) == ls.ERR_ARG


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_exact_alias_passes(ls, kind, rows, cols):
    """d_keys_out == d_keys is no overlap error.  A call that passes every check launches, which a CPU
    test must not, so the aliased call is given a workspace that is NULL or one byte short: the last
    thing looked at, and the one thing wrong with it (with the mask, without it, with d_k).  One
    element off the alias fails with a good workspace.  That the aliased call runs is
    test_gpu_topk_mask.py's in-place test."""
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    need = ls.topk_mask_workspace_bytes(rows, cols)

    def call(out, mask=3 * FAR, dk=None, wsb=BIG, ws=4 * FAR):
        return L.labsort_topk_mask_device(FAR, rows, cols, 1, dk, 1, kt, 0, out, mask, ws, wsb, None)
    for dk in (None, 5 * FAR):
        for mask in (3 * FAR, None):
            assert call(FAR, mask, dk, wsb=need - 1) == ls.ERR_ARG
            assert call(FAR, mask, dk, ws=None, wsb=need) == ls.ERR_ARG
    assert call(FAR + esz) == ls.ERR_ARG and call(FAR - esz) == ls.ERR_ARG


def test_rows_times_cols_limit(ls):
    L = ls.lib
    for kt in range(5):
        assert L.labsort_topk_mask_device(FAR, 1 << 16, 1 << 15, 1, None, 0, kt, 0, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG
        assert L.labsort_topk_mask_device(FAR, 1, 1 << 31, 1, None, 0, kt, 0, None, 1 << 50, 1 << 52, BIG, None) == ls.ERR_ARG
        assert L.labsort_topk_mask_device(FAR, 1 << 31, 1, 1, None, 1, kt, 0, FAR, None, 1 << 52, BIG, None) == ls.ERR_ARG


def test_workspace_size(ls):
    """The 256-byte header up to kth_row_keys(); above it never below the select's workspace, which it
    contains, and at most two 256-byte-aligned regions of a word per row more.  Never shrinks."""
    Rk = ls.kth_row_keys()
    for rows in (1, 3, 1000, 1 << 17):
        for cols in (1, 2, 4097, Rk - 1, Rk):
            assert ls.topk_mask_workspace_bytes(rows, cols) == 256
    assert ls.topk_mask_workspace_bytes(0, 100000) == 256 and ls.topk_mask_workspace_bytes(5, 0) == 256
    rows_grid = [1, 2, 3, 7, 64, 1000, 4096]
    cols_grid = [1, 100, Rk, Rk + 1, 2 * Rk, 2 * Rk + 1, 50257, 70001, 131072, 151936, 1 << 18, 1 << 19]
    for i, rows in enumerate(rows_grid):
        for j, cols in enumerate(cols_grid):
            w = ls.topk_mask_workspace_bytes(rows, cols)
            assert w % 256 == 0
            if i:
                assert ls.topk_mask_workspace_bytes(rows_grid[i - 1], cols) <= w
            if j:
                assert ls.topk_mask_workspace_bytes(rows, cols_grid[j - 1]) <= w
            assert ls.topk_mask_workspace_bytes(rows + 1, cols) >= w and ls.topk_mask_workspace_bytes(rows, cols + 1) >= w
            kw = ls.kth_workspace_bytes(rows, cols)
            assert w >= kw
            if cols > Rk:
                assert kw + 8 * rows <= w <= kw + 8 * rows + 2 * 256
    assert len(ls.lib.labsort_topk_mask_workspace_bytes.argtypes) == 2  # no key type


def test_python_wrappers_reject_before_the_device(ls):
    """TypeError for what kthvalue rejects and for a wrong `out`, on CPU tensors, so before any device call."""
    import torch
    for f in (ls.topk_filter, ls.topk_mask):
        for dt in (torch.bfloat16, torch.float16, torch.float32, torch.int32):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 40000), dtype=dt), 3)  # a CPU tensor
            with pytest.raises(TypeError):
                f(torch.zeros((40000, 2), dtype=dt).t(), 1)  # a transposed view
            with pytest.raises(TypeError):
                f(torch.zeros((2, 2, 100), dtype=dt), 1)
        for dt in (torch.int64, torch.float64, torch.int16, torch.uint8):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 100), dtype=dt), 1)
        with pytest.raises(TypeError):
            f(np.zeros((2, 100), dtype=np.float32), 1)
