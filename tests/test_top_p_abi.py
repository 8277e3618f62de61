"""CPU tests of the top-p filter's C ABI (labsort_top_p_*, include/labsort.h): exports, the host-side
argument checks, the one alias allowed, the empty shapes, the workspace sizing, and the checks of
ls.top_p_filter / ls.top_p_mask that come before the device.  No kernel is launched: every call below
returns before its first launch (the pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import top_p_model as P
import rowsort_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_top_p_weight", "labsort_top_p_workspace_bytes", "labsort_top_p_device", "labsort_top_p_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", P.KINDS)
SHAPES = [(4, 100), (3, 4097), (2, 16384), (2, 16385), (2, 70001)]
NAN = float("nan")


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("top_p_weight", "top_p_workspace_bytes", "top_p_device", "top_p_workspace_status", "top_p_filter", "top_p_mask"):
        assert callable(getattr(ls, f)), f
    assert hdr.index("labsort_topk_mask_device(") < hdr.index("labsort_top_p_device(") < hdr.index("labsort_unique_device(")
    assert len(ls.lib.labsort_top_p_device.argtypes) == 13
    assert len(ls.lib.labsort_top_p_workspace_bytes.argtypes) == 2  # no key type


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in (2, 3, 4, 0, 9, 77):  # (before the key type is looked at)
        assert L.labsort_top_p_device(None, 0, 10, 0.5, None, kt, 0, None, None, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_top_p_device(None, 3, 0, 0.5, None, kt, 0, None, None, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_top_p_device(FAR + 1, 0, 10, 7.0, FAR + 2, kt, 0xFFFFFFFF, FAR + 3, None, None, None, 0, None) == ls.OK


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_argument_errors(ls, kind, rows, cols):
    """Each call changes one thing of a good one (call()'s defaults: far-apart buffers, p = 0.5, a
    workspace that is large enough), so each ERR_ARG comes from the one check that the change meets.
    The workspace is the last thing looked at: the calls that differ only in it are otherwise good."""
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    nin, nm, nw = rows * cols * esz, rows * cols, rows * 4  # bytes of the keys, of the mask, of d_p and the counts
    need = ls.top_p_workspace_bytes(rows, cols)
    KEYS, OUT, MASK, KEPT, DP, WS = FAR, 2 * FAR, 3 * FAR, 4 * FAR, 5 * FAR, 6 * FAR

    def call(keys=KEYS, out=OUT, mask=MASK, kept=KEPT, dp=None, p=0.5, ws=WS, wsb=BIG, r=rows, c=cols, kt=kt, fill=0):
        return L.labsort_top_p_device(keys, r, c, p, dp, kt, fill, out, mask, kept, ws, wsb, None)
    assert call(keys=None) == ls.ERR_ARG
    assert call(out=None, mask=None, kept=None) == ls.ERR_ARG
    for bad in (0, 1, 5, 6, 7, 8, 9, 10, 11, -1):  # U32, I32; 8 .. 10: the 64-bit types
        assert call(kt=bad) == ls.ERR_ARG
    for p in (0.0, -0.0, -1.0, 1.5, NAN, float("inf"), float(np.nextafter(np.float32(1), np.float32(2)))):
        assert call(p=p) == ls.ERR_ARG
    assert call(r=1, c=(1 << 23) + 1) == ls.ERR_ARG
    assert call(r=0x7FFFFFFF // cols + 1) == ls.ERR_ARG
    # keys output against the input: one element off the exact alias either way, on its last element, behind its first
    assert call(out=KEYS + esz) == ls.ERR_ARG and call(out=KEYS - esz) == ls.ERR_ARG
    assert call(out=KEYS + nin - esz) == ls.ERR_ARG and call(out=KEYS - nin + esz) == ls.ERR_ARG
    # the mask against the input and against the keys output (also in place)
    for base in (KEYS, OUT):
        assert call(mask=base) == ls.ERR_ARG
        assert call(mask=base + nin - 1) == ls.ERR_ARG
        assert call(mask=base - nm + 1) == ls.ERR_ARG
    assert call(out=KEYS, mask=KEYS + nin - 1) == ls.ERR_ARG
    assert call(out=None, mask=KEYS + 1) == ls.ERR_ARG
    # the counts and d_p against the input, the keys output, the mask, and each other
    for base, size in ((KEYS, nin), (OUT, nin), (MASK, nm)):
        for who in ("kept", "dp"):
            assert call(**{who: base}) == ls.ERR_ARG
            assert call(**{who: base + (size - 1) // 4 * 4}) == ls.ERR_ARG
            assert call(**{who: base - nw + 4}) == ls.ERR_ARG
    assert call(out=KEYS, dp=KEYS + 4) == ls.ERR_ARG and call(out=KEYS, kept=KEYS + 4) == ls.ERR_ARG
    assert call(dp=KEPT) == ls.ERR_ARG and call(dp=KEPT + nw - 4) == ls.ERR_ARG and call(dp=KEPT - nw + 4) == ls.ERR_ARG
    assert call(kept=KEPT + 2) == ls.ERR_ARG and call(dp=DP + 1) == ls.ERR_ARG  # (not words)
    # workspace: NULL, 16 bytes short, none; with every set of outputs
    for out, mask, kept in ((OUT, MASK, KEPT), (OUT, None, None), (None, MASK, None), (None, None, KEPT), (KEYS, None, KEPT)):
        for dp_ in (None, DP):
            assert call(out=out, mask=mask, kept=kept, dp=dp_, ws=None, wsb=need) == ls.ERR_ARG
            assert call(out=out, mask=mask, kept=kept, dp=dp_, wsb=need - 16) == ls.ERR_ARG
            assert call(out=out, mask=mask, kept=kept, dp=dp_, wsb=0) == ls.ERR_ARG
    # a bad host p is not looked at when d_p is given: the short workspace is what fails, as above
    assert call(dp=DP, p=NAN, wsb=need - 1) == ls.ERR_ARG
    if esz == 2:
        assert call(keys=KEYS + 1) == ls.ERR_ARG and call(out=OUT + 1) == ls.ERR_ARG
        assert call(keys=KEYS + 1, out=KEYS + 1) == ls.ERR_ARG  # (the alias, but odd)
        for fill in (0x10000, 0xFFFF0000, 0x80000000, 0xFFFFFFFF):
            assert call(fill=fill) == ls.ERR_ARG


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_the_exact_alias_passes(ls, kind, rows, cols):
    """d_keys_out == d_keys is no overlap error.  A call that passes every check launches, which a CPU
    test must not, so the aliased call is given a workspace that is NULL or one byte short: the last
    thing looked at, and the one thing wrong with it.  One element off the alias fails with a good
    workspace.  That the aliased call runs is test_gpu_top_p.py's in-place test."""
    L, kt = ls.lib, R.KT[kind]
    esz = 2 if R.is16(kind) else 4
    need = ls.top_p_workspace_bytes(rows, cols)

    def call(out, mask=3 * FAR, kept=4 * FAR, dp=None, wsb=BIG, ws=6 * FAR):
        return L.labsort_top_p_device(FAR, rows, cols, 1.0, dp, kt, 0, out, mask, kept, ws, wsb, None)
    for dp in (None, 5 * FAR):
        for mask in (3 * FAR, None):
            for kept in (4 * FAR, None):
                assert call(FAR, mask, kept, dp, wsb=need - 1) == ls.ERR_ARG
                assert call(FAR, mask, kept, dp, ws=None, wsb=need) == ls.ERR_ARG
    assert call(FAR + esz) == ls.ERR_ARG and call(FAR - esz) == ls.ERR_ARG


def test_workspace_size(ls):
    """The 256-byte header up to kth_row_keys(); above it multiples of 256 that never shrink and hold
    at least the masses: 8 bytes per level digit and per chunk digit."""
    Rk = ls.kth_row_keys()
    for rows in (1, 3, 1000, 1 << 17):
        for cols in (1, 2, 4097, Rk - 1, Rk):
            assert ls.top_p_workspace_bytes(rows, cols) == 256
    assert ls.top_p_workspace_bytes(0, 100000) == 256 and ls.top_p_workspace_bytes(5, 0) == 256
    rows_grid = [1, 2, 3, 7, 64, 1000, 4096]
    cols_grid = [1, 100, Rk, Rk + 1, 2 * Rk, 2 * Rk + 1, 50257, 70001, 131072, 151936, 1 << 18, 1 << 19, 1 << 23]
    for i, rows in enumerate(rows_grid):
        for j, cols in enumerate(cols_grid):
            w = ls.top_p_workspace_bytes(rows, cols)
            assert w % 256 == 0
            if i:
                assert ls.top_p_workspace_bytes(rows_grid[i - 1], cols) <= w
            if j:
                assert ls.top_p_workspace_bytes(rows, cols_grid[j - 1]) <= w
            assert ls.top_p_workspace_bytes(rows + 1, cols) >= w and ls.top_p_workspace_bytes(rows, cols + 1) >= w
            if cols > Rk:
                nch = -(-cols // Rk)
                body = rows * (4 * 256 * 8 + 5 * 16 + 5 * 16 + nch * 256 * 8 + 4 + 4)
                assert 256 + body <= w <= 256 + body + 6 * 256


def test_python_wrappers_reject_before_the_device(ls):
    """TypeError on CPU tensors, wrong dtypes, views and 3-D tensors, a wrong p and a wrong `out`: all
    before any device call."""
    import torch
    for f in (ls.top_p_filter, ls.top_p_mask):
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 40000), dtype=dt), 0.5)  # a CPU tensor
            with pytest.raises(TypeError):
                f(torch.zeros((40000, 2), dtype=dt).t(), 0.5)  # a transposed view
            with pytest.raises(TypeError):
                f(torch.zeros((2, 2, 100), dtype=dt), 0.5)
        for dt in (torch.int32, torch.int64, torch.float64, torch.int16, torch.uint8):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 100), dtype=dt), 0.5)
        with pytest.raises(TypeError):
            f(np.zeros((2, 100), dtype=np.float32), 0.5)
