"""CPU tests of the segmented sort's C ABI (include/labsort.h): exports, the LDS tile
sizes and class edges, the host-side argument checks and the workspace sizing.  No
kernel is launched: every call below returns before its first launch."""
import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd", "liblabsort.so")

NAMES = ["labsort_segment_tile_keys", "labsort_segment_pair_tile_keys", "labsort_segment_class_edges",
         "labsort_segments_workspace_bytes", "labsort_sort_segments_device", "labsort_sort_segments_pairs_device",
         "labsort_segments_workspace_status"]


def test_segment_symbols_exported(ls):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    ex = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in ex, name
        assert name in ls.C_SYMBOLS, name
    assert ls.KCLASS["segsort"] == 9


def test_segment_tile_limits(ls):
    assert 4096 <= ls.segment_tile_keys() <= 32768
    assert 2048 <= ls.segment_pair_tile_keys() <= 16384


def test_segment_class_edges(ls):
    for pairs, tile in ((False, ls.segment_tile_keys()), (True, ls.segment_pair_tile_keys())):
        e = ls.segment_class_edges(pairs)
        assert len(e) >= 1 and all(a < b for a, b in zip(e, e[1:])), e
        assert e[0] >= 1 and e[-1] == tile


def test_segment_argument_errors(ls):
    L = ls.lib
    ws = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(ws)
    W = 1 << 16
    # n = 0: nothing to do, whatever else is passed
    assert L.labsort_sort_segments_device(None, None, 0, None, 0, 0, 0, None, 0, None) == ls.OK
    assert L.labsort_sort_segments_pairs_device(None, None, None, None, 0, None, 0, 0, 0, None, 0, None) == ls.OK
    # NULL keys
    assert L.labsort_sort_segments_device(None, None, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_device(p, p + 64, 10, None, 1, 10, 0, p + 4096, W - 4096, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_pairs_device(None, p, None, p, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_pairs_device(p, None, p + 64, None, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    # bad key type
    assert L.labsort_sort_segments_device(p, p, 10, p, 1, 10, 7, p, W, None) == ls.ERR_ARG
    # no segments for 10 keys
    assert L.labsort_sort_segments_device(p, p, 10, p, 0, 10, 0, p, W, None) == ls.ERR_ARG
    # workspace missing / 16 bytes too small, on both paths
    for n, nseg, m, pairs in ((1000, 10, 100, 0), (1000, 10, 100, 1), (1000, 10, 0, 0), (1000, 10, 0, 1)):
        need = L.labsort_segments_workspace_bytes(n, nseg, m, pairs)
        big = ctypes.create_string_buffer(need + 4 * 4096)
        q = ctypes.addressof(big)
        if pairs:
            assert L.labsort_sort_segments_pairs_device(q, q + 4096, q + 8192, q + 12288, n, q, nseg, m, 0, q, need - 16,
                                                        None) == ls.ERR_ARG
            assert L.labsort_sort_segments_pairs_device(q, q + 4096, q + 8192, q + 12288, n, q, nseg, m, 0, None, need,
                                                        None) == ls.ERR_ARG
        else:
            assert L.labsort_sort_segments_device(q, q + 4096, n, q, nseg, m, 0, q, need - 16, None) == ls.ERR_ARG
            assert L.labsort_sort_segments_device(q, q + 4096, n, q, nseg, m, 0, None, need, None) == ls.ERR_ARG
    # pairs: one side aliased and the other not
    assert L.labsort_sort_segments_pairs_device(p, p + 64, p, p + 128, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_pairs_device(p, p + 64, p + 128, p + 64, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_pairs_device(p, p + 64, p + 128, p + 128, 10, p, 1, 10, 0, p, W, None) == ls.ERR_ARG
    # general path beyond the radix limit (the workspace argument is never reached)
    assert ls.max_keys("radix") == (1 << 30) - 1
    assert L.labsort_sort_segments_device(p, p, 1 << 30, p, 1, 0, 0, p, 1 << 62, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_pairs_device(p, p + 64, p, p + 64, 1 << 30, p, 1, 0, 0, p, 1 << 62, None) == ls.ERR_ARG
    # n beyond 2^31 - 1 on the LDS path
    assert L.labsort_sort_segments_device(p, p, 1 << 31, p, 1 << 20, 4096, 0, p, 1 << 62, None) == ls.ERR_ARG


def test_segments_workspace_size(ls):
    T, TP = ls.segment_tile_keys(), ls.segment_pair_tile_keys()
    ns = [1, 100, TP, TP + 1, T, T + 1, 1 << 16, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, 1 << 20, 1 << 25, (1 << 25) + 1,
          1 << 28, (1 << 30) - 1]
    segs = [1, 2, 63, 64, 65, 1000, 4096, 4097, 1 << 18, 1 << 24]
    for pairs in (False, True):
        for m in (1, 16, 300, 4096, TP, 0, T + 1, 1 << 20):  # LDS path and general path
            for nseg in (1, 1000):
                w = [ls.segments_workspace_bytes(n, nseg, m, pairs) for n in ns]
                assert w == sorted(w), (pairs, m, nseg, w)
            for n in (1000, 1 << 20):
                w = [ls.segments_workspace_bytes(n, nseg, m, pairs) for nseg in segs]
                assert w == sorted(w), (pairs, m, n, w)
        # LDS path: O(nseg), no term in n
        assert ls.segments_workspace_bytes(1 << 28, 1 << 18, 1024, pairs) <= 64 * (1 << 18) + 65536
        for nseg in segs:
            assert ls.segments_workspace_bytes(1 << 28, nseg, 16, pairs) <= 64 * nseg + 65536
            assert ls.segments_workspace_bytes(1 << 28, nseg, 16, pairs) == ls.segments_workspace_bytes(5, nseg, 16, pairs)
        # general path: two n-word buffers at the very least
        for n in ns:
            assert ls.segments_workspace_bytes(n, 10, 0, pairs) >= 8 * n
            assert ls.segments_workspace_bytes(n, 10, (TP if pairs else T) + 1, pairs) >= 8 * n
    # the pair tile is the smaller: a length between the two tiles is LDS for keys, general for pairs
    if TP < T:
        assert ls.segments_workspace_bytes(1 << 20, 10, T, False) < 8 * (1 << 20)
        assert ls.segments_workspace_bytes(1 << 20, 10, T, True) >= 8 * (1 << 20)
