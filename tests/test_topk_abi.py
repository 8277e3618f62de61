"""CPU tests of the top-k selection's C ABI (include/labsort.h): exports, the timing class,
the host-side argument checks and the workspace sizing.  No kernel is launched: every call
below returns before its first launch."""
import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")

NAMES = ["labsort_topk_workspace_bytes", "labsort_topk_device", "labsort_topk_workspace_status"]


def test_topk_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
    assert ls.KCLASS["topk"] == 10
    ms, cnt = ctypes.c_double(-1.0), ctypes.c_longlong(-1)
    assert ls.lib.labsort_timing_read(10, ctypes.byref(ms), ctypes.byref(cnt)) == ls.OK
    assert ls.lib.labsort_timing_read(11, ctypes.byref(ms), ctypes.byref(cnt)) == ls.ERR_ARG
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    assert "#define LABSORT_K_TOPK 10" in hdr and "#define LABSORT_K_COUNT 11" in hdr
    assert "#define LABSORT_TOPK_SORT_DIV %d" % ls.TOPK_SORT_DIV in hdr


def test_topk_nothing_to_do(ls):
    L = ls.lib
    assert L.labsort_topk_device(None, 0, 10, 5, 0, 0, None, None, None, 0, None) == ls.OK  # rows == 0
    assert L.labsort_topk_device(None, 3, 10, 0, 1, 1, None, None, None, 0, None) == ls.OK  # k == 0
    assert L.labsort_topk_device(None, 0, 0, 0, 0, 0, None, None, None, 0, None) == ls.OK


def test_topk_argument_errors(ls):
    L = ls.lib
    TP = ls.segment_pair_tile_keys()
    # (rows, cols, k): the short path, the select and the whole-row sort
    for rows, cols, k in ((4, 100, 7), (2, TP + 100, 9), (1, TP + 100, 9), (2, TP + 100, TP)):
        need = L.labsort_topk_workspace_bytes(rows, cols, k)
        assert need >= 256
        nin, nout = rows * cols * 4, rows * k * 4
        buf = ctypes.create_string_buffer(nin + 2 * nout + need + 1024)
        q = ctypes.addressof(buf)
        q += (-q) % 256
        kin, kout, iout, ws = q, q + nin, q + nin + nout, q + nin + 2 * nout
        ws += (-ws) % 256

        def call(kin=kin, rows=rows, cols=cols, k=k, largest=0, kt=0, kout=kout, iout=iout, ws=ws, wsb=need):
            return L.labsort_topk_device(kin, rows, cols, k, largest, kt, kout, iout, ws, wsb, None)

        assert call(kin=None) == ls.ERR_ARG  # NULL keys
        assert call(kout=None) == ls.ERR_ARG  # NULL output
        assert call(kt=7) == ls.ERR_ARG and call(kt=-1) == ls.ERR_ARG  # bad key type
        assert call(k=cols + 1, wsb=1 << 62) == ls.ERR_ARG  # k > cols
        assert call(ws=None) == ls.ERR_ARG  # workspace missing
        assert call(wsb=need - 16) == ls.ERR_ARG  # 16 bytes too small
        assert call(wsb=0) == ls.ERR_ARG
        assert call(kout=kin) == ls.ERR_ARG  # output over the input
        assert call(kout=kin + nin - 4) == ls.ERR_ARG  # ... over its last word
        assert call(kout=kin - nout + 4) == ls.ERR_ARG  # ... over its first word
        assert call(iout=kin + 8) == ls.ERR_ARG  # indices over the input
        assert call(iout=kout) == ls.ERR_ARG  # indices == keys out
    p = q
    # rows * cols beyond 2^31 - 1
    assert L.labsort_topk_device(p, 1 << 16, 1 << 15, 4, 0, 0, p, None, p, 1 << 62, None) == ls.ERR_ARG
    assert L.labsort_topk_device(p, 1, 1 << 31, 4, 0, 0, p, None, p, 1 << 62, None) == ls.ERR_ARG
    # several rows whose survivors the segmented sort's general path cannot order: k beyond the
    # pair tile and rows * k beyond the radix limit (the pointers are far apart; nothing is launched)
    maxr = ls.max_keys("radix")
    rows, cols = 3, (2**31 - 1) // 3
    k = maxr // rows + 1
    assert k > TP and rows * k > maxr and k <= cols
    far = 1 << 40
    assert L.labsort_topk_device(far, rows, cols, k, 0, 0, 2 * far, None, 3 * far, 1 << 62, None) == ls.ERR_ARG


def test_topk_workspace_size(ls):
    TP = ls.segment_pair_tile_keys()
    D = ls.TOPK_SORT_DIV
    # rows shorter and longer than the pair tile; ks on both sides of cols // D
    for rows in (1, 3, 1000):
        for cols in (1, 5, 4096, TP, TP + 1, 70001, 1 << 20, (1 << 21) + 3):
            if rows * cols >= 2**31:
                continue
            ks = sorted({k for k in (1, 2, 64, 1000, TP, TP + 1, cols // D, cols // D + 1, cols // 2, cols - 1, cols)
                         if 1 <= k <= cols})
            w = [ls.topk_workspace_bytes(rows, cols, k) for k in ks]
            assert w == sorted(w), (rows, cols, list(zip(ks, w)))
            assert all(x >= 256 for x in w)
    assert ls.topk_workspace_bytes(0, 10, 5) <= 256 and ls.topk_workspace_bytes(3, 10, 0) <= 256
    # a select does not need sort-sized scratch: for small k, less than 8 bytes per key plus a fixed
    # slack (the header, a few KiB of tables per row, the survivors' buffers and their sort)
    slack = 1 << 20
    for rows, cols in ((1, TP + 1), (1, 70001), (1, 1 << 22), (1, 1 << 28), (5, 3 * 16384 + 7), (4096, 1 << 16),
                       (1 << 12, (1 << 16) + 1)):
        for k in (1, 64, 1000):
            w = ls.topk_workspace_bytes(rows, cols, k)
            assert w < 8 * rows * cols + slack, (rows, cols, k, w)
    # and at the headline shape well below a sort's: under 2 bytes per key
    assert ls.topk_workspace_bytes(1, 1 << 28, 1024) < 2 * (1 << 28)
    # whole-row sorting (k above the threshold) holds the pairs twice at the least
    assert ls.topk_workspace_bytes(1, 1 << 20, 1 << 19) >= 16 * (1 << 20)
