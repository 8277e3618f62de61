"""CPU tests of categorical sampling's C ABI (labsort_sample_*, include/labsort.h): exports, the empty
shapes, the host-side argument checks, the workspace sizing, and the checks of ls.sample that come
before the device.  No kernel is launched: every call below returns before its first launch (the
pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import rowsort_model as R
import top_p_model as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_sample_workspace_bytes", "labsort_sample_device", "labsort_sample_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", P.KINDS)
SHAPES = [(4, 100, 1), (3, 4097, 5), (2, 16384, 1000), (2, 16385, 1), (2, 70001, 7)]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("sample_workspace_bytes", "sample_device", "sample_workspace_status", "sample"):
        assert callable(getattr(ls, f)), f
    assert hdr.index("labsort_top_p_device(") < hdr.index("labsort_sample_device(") < hdr.index("labsort_unique_device(")
    assert hdr.index("labsort_top_p_workspace_status(") < hdr.index("labsort_sample_workspace_bytes(")
    assert "floor or ceil of w 2^32 / W_r values of U" in " ".join(hdr.replace("*", " ").split())
    assert len(ls.lib.labsort_sample_device.argtypes) == 10
    assert len(ls.lib.labsort_sample_workspace_bytes.argtypes) == 3  # no key type
    assert len(ls.lib.labsort_sample_workspace_status.argtypes) == 2


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in (2, 3, 4, 0, 9, 77):  # (before the key type is looked at)
        assert L.labsort_sample_device(None, 0, 10, None, 3, kt, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_sample_device(None, 3, 0, None, 3, kt, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_sample_device(None, 3, 10, None, 0, kt, None, None, 0, None) == ls.OK  # ndraw == 0
        assert L.labsort_sample_device(FAR + 1, 0, 1 << 30, FAR + 2, 1 << 40, kt, FAR + 3, None, 0, None) == ls.OK
        assert L.labsort_sample_device(FAR + 1, 5, 1 << 30, FAR + 1, 0, kt, FAR + 1, None, 0, None) == ls.OK


@KINDS
@pytest.mark.parametrize("rows,cols,ndraw", SHAPES)
def test_argument_errors(ls, kind, rows, cols, ndraw):
    """Each call changes one thing of a good one (call()'s defaults: far-apart buffers and a workspace
    that is large enough), so each ERR_ARG comes from the one check that the change meets.  The
    workspace is the last thing looked at: the calls that differ only in it are otherwise good."""
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    nin, nw = rows * cols * esz, rows * ndraw * 4  # bytes of the keys, of the words and of the positions
    need = ls.sample_workspace_bytes(rows, cols, ndraw)
    KEYS, U, OUT, WS = FAR, 2 * FAR, 3 * FAR, 6 * FAR

    def call(keys=KEYS, u=U, out=OUT, ws=WS, wsb=BIG, r=rows, c=cols, nd=ndraw, kt=kt):
        return L.labsort_sample_device(keys, r, c, u, nd, kt, out, ws, wsb, None)
    assert call(keys=None) == ls.ERR_ARG and call(u=None) == ls.ERR_ARG and call(out=None) == ls.ERR_ARG
    for bad in (0, 1, 5, 6, 7, 8, 9, 10, 11, -1):  # U32, I32; 8 .. 10: the 64-bit types
        assert call(kt=bad) == ls.ERR_ARG
    assert call(r=1, c=(1 << 23) + 1) == ls.ERR_ARG
    assert call(r=0x7FFFFFFF // cols + 1, nd=1) == ls.ERR_ARG
    assert call(r=0x7FFFFFFF // ndraw + 1, c=1) == ls.ERR_ARG
    assert call(r=2, c=1, nd=1 << 30) == ls.ERR_ARG
    if esz == 2:
        assert call(keys=KEYS + 1) == ls.ERR_ARG
    for off in (1, 2, 3):  # (not words)
        assert call(u=U + off) == ls.ERR_ARG and call(out=OUT + off) == ls.ERR_ARG
    # the words and the positions against the input: on its first element, on its last, ending on its first
    for who in ("u", "out"):
        assert call(**{who: KEYS}) == ls.ERR_ARG
        assert call(**{who: KEYS + (nin - 1) // 4 * 4}) == ls.ERR_ARG
        assert call(**{who: KEYS - nw + 4}) == ls.ERR_ARG
    # the words against the positions: the same buffer, one word inside it either way
    assert call(out=U) == ls.ERR_ARG and call(out=U + nw - 4) == ls.ERR_ARG and call(out=U - nw + 4) == ls.ERR_ARG
    # workspace: NULL, 16 bytes short, none
    assert call(ws=None, wsb=need) == ls.ERR_ARG
    assert call(wsb=need - 16) == ls.ERR_ARG and call(wsb=need - 1) == ls.ERR_ARG and call(wsb=0) == ls.ERR_ARG
    # buffers that touch without sharing a byte are no overlap: the short workspace is what fails
    assert call(u=KEYS + (nin + 3) // 4 * 4, out=KEYS - nw, wsb=need - 1) == ls.ERR_ARG


def test_workspace_size(ls):
    """The 256-byte header up to kth_row_keys(); above it the header, rows x chunks 8-byte masses and
    rows x ndraw 16-byte draw states, each region 256-byte aligned; never shrinking in any argument."""
    Rk = ls.kth_row_keys()
    assert Rk == 16384
    for rows in (1, 3, 1000, 1 << 17):
        for cols in (1, 2, 4097, Rk - 1, Rk):
            for nd in (1, 8, 1000):
                assert ls.sample_workspace_bytes(rows, cols, nd) == 256
    assert ls.sample_workspace_bytes(0, 100000, 1) == 256 and ls.sample_workspace_bytes(5, 0, 1) == 256
    assert ls.sample_workspace_bytes(5, 100000, 0) == 256

    def up(v):
        return -(-v // 256) * 256
    rows_grid = [1, 2, 3, 7, 64, 1000, 4096]
    cols_grid = [1, 100, Rk, Rk + 1, 2 * Rk, 2 * Rk + 1, 50257, 70001, 131072, 151936, 1 << 18, 1 << 19, 1 << 23]
    nd_grid = [1, 2, 5, 16, 17, 1000]
    for i, rows in enumerate(rows_grid):
        for j, cols in enumerate(cols_grid):
            for k, nd in enumerate(nd_grid):
                w = ls.sample_workspace_bytes(rows, cols, nd)
                assert w % 256 == 0
                if i:
                    assert ls.sample_workspace_bytes(rows_grid[i - 1], cols, nd) <= w
                if j:
                    assert ls.sample_workspace_bytes(rows, cols_grid[j - 1], nd) <= w
                if k:
                    assert ls.sample_workspace_bytes(rows, cols, nd_grid[k - 1]) <= w
                assert ls.sample_workspace_bytes(rows + 1, cols, nd) >= w and ls.sample_workspace_bytes(rows, cols + 1, nd) >= w
                assert ls.sample_workspace_bytes(rows, cols, nd + 1) >= w
                if cols > Rk:
                    assert w == 256 + up(rows * -(-cols // Rk) * 8) + up(rows * nd * 16)


def test_python_wrapper_rejects_before_the_device(ls):
    """TypeError on CPU tensors, wrong dtypes, views and 3-D tensors: all before any device call.  (The
    checks of num_samples and u come after x's and need a CUDA x: test_gpu_sample.py has them.)"""
    import torch
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(TypeError):
            ls.sample(torch.zeros((2, 40000), dtype=dt))  # a CPU tensor
        with pytest.raises(TypeError):
            ls.sample(torch.zeros((40000, 2), dtype=dt).t())  # a transposed view
        with pytest.raises(TypeError):
            ls.sample(torch.zeros((2, 2, 100), dtype=dt))
    for dt in (torch.int32, torch.int64, torch.float64, torch.int16, torch.uint8):
        with pytest.raises(TypeError):
            ls.sample(torch.zeros((2, 100), dtype=dt))
    with pytest.raises(TypeError):
        ls.sample(np.zeros((2, 100), dtype=np.float32))
