"""CPU tests of the 16-bit sort's C ABI (labsort_sort16_*, include/labsort.h): exports, the key types it
takes, the host-side argument checks of the dense row sort applied to it, the workspace sizing, and
ls.sort's checks that come before the device.  No kernel is launched: every call below returns before
its first launch (the pointers are made-up addresses, far apart)."""
import os
import subprocess

import numpy as np
import pytest

import f16_model as M
import rowsort_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")
NAMES = ["labsort_sort16_chunk_keys", "labsort_sort16_workspace_bytes", "labsort_sort16_device",
         "labsort_sort16_workspace_status"]
FAR = 1 << 40
BIG = 1 << 62
KINDS = pytest.mark.parametrize("kind", M.KINDS)
# the LDS path's wave, block and tile classes, the edge of the tile, the long path
SHAPES = [(4, 100), (3, 4097), (2, 16385), (2, 32768), (2, 32769), (2, 70001)]
LONG_SHAPES = [(1, 32769), (2, 70001), (5216, 50257), (2048, 131072), (1, 1 << 28)]


def test_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
        assert name + "(" in hdr, name
    for f in ("sort16_chunk_keys", "sort16_workspace_bytes", "sort16_device", "sort16_workspace_status"):
        assert callable(getattr(ls, f)), f
    c = ls.sort16_chunk_keys()
    assert 1024 <= c <= 65536 and c % 64 == 0


def test_nothing_to_do(ls):
    L = ls.lib
    for kt in (R.KT["bf16"], R.KT["f16"]):
        assert L.labsort_sort16_device(None, 0, 10, 0, kt, None, None, None, 0, None) == ls.OK  # rows == 0
        assert L.labsort_sort16_device(None, 3, 0, 1, kt, None, None, None, 0, None) == ls.OK  # cols == 0
        assert L.labsort_sort16_device(None, 0, 0, 0, kt, None, None, None, 0, None) == ls.OK
        assert L.labsort_sort16_device(FAR + 1, 0, 10, 1, kt, FAR + 3, None, None, 0, None) == ls.OK


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_other_key_types_rejected(ls, rows, cols):
    """U32, I32, F32, the unknown 5 and 7, and -1, with otherwise good arguments."""
    L = ls.lib
    for kt in (0, 1, 2, 5, 7, -1):
        for desc in (0, 1):
            for idx in (3 * FAR, None):
                assert L.labsort_sort16_device(FAR, rows, cols, desc, kt, 2 * FAR, idx, 4 * FAR, BIG, None) == ls.ERR_ARG


@KINDS
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_argument_errors(ls, kind, rows, cols):
    L, kt = ls.lib, R.KT[kind]
    esz = 2
    nin = rows * cols * esz  # bytes of the input and of the key output
    nidx = rows * cols * 4
    for desc in (0, 1):
        def call(keys=FAR, out=2 * FAR, idx=3 * FAR, ws=4 * FAR, wsb=BIG, r=rows, c=cols, kt=kt):
            return L.labsort_sort16_device(keys, r, c, desc, kt, out, idx, ws, wsb, None)
        assert call(keys=None) == ls.ERR_ARG and call(out=None) == ls.ERR_ARG
        assert call(r=0x7FFFFFFF // cols + 1) == ls.ERR_ARG  # rows * cols past 2^31 - 1
        assert call(idx=2 * FAR) == ls.ERR_ARG  # d_idx_out == d_keys_out
        # overlap by the real extents: on the input's last and first element, and the whole of it
        assert call(out=FAR + nin - esz) == ls.ERR_ARG
        assert call(out=FAR - nin + esz) == ls.ERR_ARG
        assert call(out=FAR) == ls.ERR_ARG
        assert call(idx=FAR + nin - 4) == ls.ERR_ARG
        assert call(idx=FAR - nidx + 4) == ls.ERR_ARG
        assert call(idx=FAR) == ls.ERR_ARG
        # workspace: NULL, 16 bytes short, none; with and without positions
        for idx in (3 * FAR, None):
            need = ls.sort16_workspace_bytes(rows, cols, idx is not None)
            assert call(idx=idx, ws=None, wsb=need) == ls.ERR_ARG
            assert call(idx=idx, wsb=need - 16) == ls.ERR_ARG
            assert call(idx=idx, wsb=0) == ls.ERR_ARG
        # odd addresses
        assert call(keys=FAR + 1) == ls.ERR_ARG and call(out=2 * FAR + 1) == ls.ERR_ARG
        assert call(keys=FAR + 1, out=2 * FAR + 1) == ls.ERR_ARG
        # an output directly behind the input, which 4-byte extents would reject, gets past the
        # overlap checks and fails only on the (deliberately) NULL workspace ...
        assert call(out=FAR + nin, ws=None) == ls.ERR_ARG
        assert call(out=FAR - nin, idx=FAR + nin, ws=None) == ls.ERR_ARG
    # ... which is the one thing wrong with it: an overlap would have been reported for any
    # workspace (shown above with a good one)


def test_rows_times_cols_limit(ls):
    L = ls.lib
    for kt in (R.KT["bf16"], R.KT["f16"]):
        assert L.labsort_sort16_device(FAR, 1 << 16, 1 << 15, 0, kt, 2 * FAR, None, 3 * FAR, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort16_device(FAR, 1, 1 << 31, 0, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort16_device(FAR, 1 << 31, 1, 1, kt, 1 << 50, None, 1 << 52, BIG, None) == ls.ERR_ARG


def test_workspace_size(ls):
    """The 256-byte header up to the tile; above it the temporaries of the two passes and the count
    table: at least 6 (2) bytes per key, and less than the row sort's route needs."""
    T = ls.segment_tile_keys()
    assert T == 32768
    for rows in (1, 3, 1000):
        for cols in (1, 16384, 16385, T):
            for pos in (True, False):
                assert ls.sort16_workspace_bytes(rows, cols, pos) == 256
    assert ls.sort16_workspace_bytes(0, 100000) == 256 and ls.sort16_workspace_bytes(5, 0) == 256
    for rows, cols in LONG_SHAPES:
        n = rows * cols
        w1, w0 = ls.sort16_workspace_bytes(rows, cols, True), ls.sort16_workspace_bytes(rows, cols, False)
        assert w1 >= 6 * n + 256 and w0 >= 2 * n + 256
        assert w0 <= w1
        assert w1 < ls.sort_rows_workspace_bytes(rows, cols)
        assert w1 % 256 == 0 and w0 % 256 == 0
        for pos in (True, False):  # never shrinks as rows or cols grow
            w = ls.sort16_workspace_bytes(rows, cols, pos)
            assert ls.sort16_workspace_bytes(rows + 1, cols, pos) >= w
            assert ls.sort16_workspace_bytes(rows, cols + 1, pos) >= w
            assert ls.sort16_workspace_bytes(rows, cols - 1, pos) <= w
            if rows > 1:
                assert ls.sort16_workspace_bytes(rows - 1, cols, pos) <= w
    assert ls.sort16_workspace_bytes(1, T + 1, True) > ls.sort16_workspace_bytes(1000, T, True)
    assert len(ls.lib.labsort_sort16_workspace_bytes.argtypes) == 3


def test_sort_rejects_other_inputs_before_the_device(ls):
    """ls.sort / ls.argsort with the new route in place: TypeError for a CPU tensor, a dtype that is no
    key type and a non-contiguous tensor, on CPU tensors, so before any device call -- rows past the
    tile, which the new route would take, included."""
    import torch
    for f in (ls.sort, ls.argsort):
        for dt in (torch.bfloat16, torch.float16, torch.float32, torch.int32):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 40000), dtype=dt))  # a CPU tensor
            with pytest.raises(TypeError):
                f(torch.zeros(40000, dtype=dt))
            with pytest.raises(TypeError):
                f(torch.zeros((40000, 2), dtype=dt).t())  # a transposed view
            with pytest.raises(TypeError):
                f(torch.zeros((2, 2, 40000), dtype=dt))
        for dt in (torch.int64, torch.float64, torch.int16, torch.uint8):
            with pytest.raises(TypeError):
                f(torch.zeros((2, 40000), dtype=dt))
        with pytest.raises(TypeError):
            f(np.zeros((2, 40000), dtype=np.float16))
