"""CPU tests of the dense row sort's C ABI (labsort_sort_rows_*, include/labsort.h): exports, the
host-side argument checks for every key type, the workspace sizing, and ls.sort's checks that come
before the device.  No kernel is launched: every call below returns before its first launch (the
pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import rowsort_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_sort_rows_workspace_bytes", "labsort_sort_rows_device", "labsort_sort_rows_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", R.KINDS)
# the LDS path's wave, block and tile classes, the edges of the two tiles, the long path
SHAPES = [(4, 100), (3, 4097), (2, 16384), (2, 16385), (2, 32768), (2, 32769), (2, 70001)]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("sort_rows_workspace_bytes", "sort_rows_device", "sort_rows_workspace_status", "sort", "argsort"):
        assert callable(getattr(ls, f)), f


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in list(R.KT.values()) + [7, -1]:  # before anything is looked at, the key type included
        assert L.labsort_sort_rows_device(None, 0, 10, 0, kt, None, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_sort_rows_device(None, 3, 0, 1, kt, None, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_sort_rows_device(None, 0, 0, 0, kt, None, None, None, 0, None) == ls.OK
        assert L.labsort_sort_rows_device(FAR + 1, 0, 10, 1, kt, FAR + 3, None, None, 0, None) == ls.OK


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_argument_errors(ls, kind, rows, cols):
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    nin = rows * cols * esz  # bytes of the input and of the key output
    nidx = rows * cols * 4
    need = ls.sort_rows_workspace_bytes(rows, cols)
    for desc in (0, 1):
        def call(keys=FAR, out=2 * FAR, idx=3 * FAR, ws=4 * FAR, wsb=BIG, r=rows, c=cols, kt=kt):
            return L.labsort_sort_rows_device(keys, r, c, desc, kt, out, idx, ws, wsb, None)
        assert call(keys=None) == ls.ERR_ARG and call(out=None) == ls.ERR_ARG
        assert call(kt=7) == ls.ERR_ARG and call(kt=-1) == ls.ERR_ARG
        assert call(r=0x7FFFFFFF // cols + 1) == ls.ERR_ARG  # rows * cols past 2^31 - 1
        assert call(idx=2 * FAR) == ls.ERR_ARG  # d_idx_out == d_keys_out
        # overlap by the real extents: on the input's last and first element, and the whole of it
        assert call(out=FAR + nin - esz) == ls.ERR_ARG
        assert call(out=FAR - nin + esz) == ls.ERR_ARG
        assert call(out=FAR) == ls.ERR_ARG
        assert call(idx=FAR + nin - 4) == ls.ERR_ARG
        assert call(idx=FAR - nidx + 4) == ls.ERR_ARG
        assert call(idx=FAR) == ls.ERR_ARG
        # workspace: NULL, 16 bytes short, none; with and without indices
        for idx in (3 * FAR, None):
            assert call(idx=idx, ws=None, wsb=need) == ls.ERR_ARG
            assert call(idx=idx, wsb=need - 16) == ls.ERR_ARG
            assert call(idx=idx, wsb=0) == ls.ERR_ARG
        if R.is16(kind):
            assert call(keys=FAR + 1) == ls.ERR_ARG and call(out=2 * FAR + 1) == ls.ERR_ARG
            assert call(keys=FAR + 1, out=2 * FAR + 1) == ls.ERR_ARG
            # an output directly behind the input, which 4-byte extents would reject, gets past the
            # overlap checks and fails only on the (deliberately) NULL workspace ...
            assert call(out=FAR + nin, ws=None) == ls.ERR_ARG
            assert call(out=FAR - nin, idx=FAR + nin, ws=None) == ls.ERR_ARG
    # ... which is the one thing wrong with it: rows == 0 returns OK earlier, and an overlap
    # would have been reported for any workspace (shown above with a good one)


def test_rows_times_cols_limit(ls):
    L = ls.lib
    for kt in R.KT.values():
        assert L.labsort_sort_rows_device(FAR, 1 << 16, 1 << 15, 0, kt, 2 * FAR, None, 3 * FAR, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort_rows_device(FAR, 1, 1 << 31, 0, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort_rows_device(FAR, 1 << 31, 1, 1, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG


def test_workspace_size(ls):
    """256 bytes up to the pair tile, top-k's size with k = cols above it; no key type in the signature."""
    TP = ls.segment_pair_tile_keys()
    assert TP == 16384 and ls.segment_tile_keys() == 32768
    for rows in (1, 3, 1000):
        for cols in (1, 16384):
            assert ls.sort_rows_workspace_bytes(rows, cols) == 256
        for cols in (16385, 70001):
            w = ls.sort_rows_workspace_bytes(rows, cols)
            assert w == ls.topk_workspace_bytes(rows, cols, cols) and w > 256
    assert ls.sort_rows_workspace_bytes(0, 100) == 256 and ls.sort_rows_workspace_bytes(5, 0) == 256
    assert len(ls.lib.labsort_sort_rows_workspace_bytes.argtypes) == 2
    import re
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    assert re.search(r"size_t labsort_sort_rows_workspace_bytes\(size_t rows, size_t cols\);", hdr)


def test_sort_rejects_other_inputs_before_the_device(ls):
    """ls.sort / ls.argsort: TypeError for a CPU tensor, a dtype that is no key type and a
    non-contiguous tensor, on CPU tensors, so before any device call."""
    import torch
    for f in (ls.sort, ls.argsort):
        for dt in (torch.float32, torch.bfloat16, torch.float16, torch.int32):
            with pytest.raises(TypeError):
                f(torch.zeros((4, 8), dtype=dt))  # a CPU tensor
            with pytest.raises(TypeError):
                f(torch.zeros((8, 4), dtype=dt).t())  # a transposed view
            with pytest.raises(TypeError):
                f(torch.zeros((2, 4, 8), dtype=dt))
        for dt in (torch.int64, torch.float64, torch.int16, torch.uint8):
            with pytest.raises(TypeError):
                f(torch.zeros((4, 8), dtype=dt))
        with pytest.raises(TypeError):
            f(np.zeros((4, 8), dtype=np.float32))
