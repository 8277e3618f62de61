"""CPU tests of the float32 key type (LABSORT_KEY_F32, include/labsort.h): the order map the
kernels compile, pinned through labsort_key_order_bits / labsort_key_from_order_bits against the
numpy model; which entries accept key type 2 and which keep rejecting it; workspace sizes unchanged
from the commit before the key type existed.  No kernel is launched: every device entry called
below returns before its first launch."""
import ctypes
import json
import os
import struct

import numpy as np

import f32_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "f32_workspace_sizes.json")
F32 = 2


def lib_map(ls, words, key, inverse=False):
    f = ls.lib.labsort_key_from_order_bits if inverse else ls.lib.labsort_key_order_bits
    return np.array([f(int(w), ls.KEY[key]) for w in words], dtype=np.uint32)


def test_key_type_constant(ls):
    assert ls.KEY["f32"] == F32 and ls.KEY["u32"] == 0 and ls.KEY["i32"] == 1
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    assert "#define LABSORT_KEY_F32 2" in hdr
    for name in ("labsort_key_order_bits", "labsort_key_from_order_bits"):
        assert name in ls.C_SYMBOLS


def test_order_bits_specials(ls):
    words = M.PLANTED
    np.testing.assert_array_equal(lib_map(ls, words, "f32"), M.ord_bits(words))
    S = M.SPECIALS
    o = {k: ls.key_order_bits(v, "f32") for k, v in S.items()}
    assert o["qnan"] == o["-qnan1"] == o["snan"] == 0xFFFFFFFF
    assert (o["-inf"] < o["-flt_max"] < o["-denorm_min"] < o["-0"] < o["+0"] < o["+denorm_min"] < o["+flt_max"]
            < o["+inf"] < o["qnan"])
    assert o["-0"] + 1 == o["+0"]
    assert o["-inf"] == 0x007FFFFF and o["+inf"] == 0xFF800000
    # the NaN image comes back as a NaN: 0x7FFFFFFF
    assert ls.key_from_order_bits(0xFFFFFFFF, "f32") == 0x7FFFFFFF
    assert M.is_nan(np.uint32(0x7FFFFFFF))


def test_order_bits_random_words(ls):
    x = M.random_words((100000,), 0xF32A)
    assert 200 < int(M.is_nan(x).sum()) < 700  # about 0.4 %
    o = lib_map(ls, x, "f32")
    np.testing.assert_array_equal(o, M.ord_bits(x))
    back = lib_map(ls, o, "f32", inverse=True)
    np.testing.assert_array_equal(back, M.unord_bits(o))
    ok = ~M.is_nan(x)
    np.testing.assert_array_equal(back[ok], x[ok])        # the round trip of every non-NaN word
    assert np.all(back[~ok] == 0x7FFFFFFF)
    # monotone: plain uint32 order of the image is the float order of the non-NaN words (-0.0 == +0.0
    # as floats: the image may order them, never against a strict float inequality)
    w, ow = x[ok], o[ok]
    p = np.argsort(ow, kind="stable")
    f = w[p].view(np.float32)
    assert np.all(f[:-1] <= f[1:])
    q = np.argsort(w.view(np.float32), kind="stable")
    fs, os_ = w[q].view(np.float32), ow[q].astype(np.int64)
    strict = fs[:-1] < fs[1:]
    assert np.all(os_[:-1][strict] < os_[1:][strict])


def test_order_bits_integer_types(ls):
    x = M.random_words((2000,), 0xF32B)
    np.testing.assert_array_equal(lib_map(ls, x, "u32"), x)
    np.testing.assert_array_equal(lib_map(ls, x, "i32"), x ^ np.uint32(0x80000000))
    np.testing.assert_array_equal(lib_map(ls, x, "u32", inverse=True), x)
    np.testing.assert_array_equal(lib_map(ls, x, "i32", inverse=True), x ^ np.uint32(0x80000000))
    # the image of an int32 orders as the int32
    s = x.view(np.int32)
    p = np.argsort(lib_map(ls, x, "i32"), kind="stable")
    assert np.all(s[p][:-1] <= s[p][1:])
    assert struct.unpack("<f", struct.pack("<I", ls.key_from_order_bits(ls.key_order_bits(0x3F800000, "f32"), "f32")))[0] == 1.0


def _buffers():
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 256
    return buf, p


def test_entries_that_reject_f32(ls):
    """key_type_ok() stays integer-only: the host-pointer sort, the run merge and the bound query
    return ERR_ARG for key type 2 before any HIP call."""
    L = ls.lib
    buf, p = _buffers()
    for kt in (F32, 7, -1):
        assert L.labsort_sort_host(p, 100, kt, ls.ALGO["auto"]) == ls.ERR_ARG
        offs = (ctypes.c_size_t * 3)(0, 0, 0)  # two empty runs: OK for a good key type, nothing launched
        assert L.labsort_merge_runs(p, p + 4096, offs, 2, kt, p + 8192, 4096, None) == ls.ERR_ARG
        assert L.labsort_upper_bound(p, 10, kt, p + 4096, 4, p + 8192, None) == ls.ERR_ARG
    offs = (ctypes.c_size_t * 3)(0, 0, 0)
    assert L.labsort_merge_runs(p, p + 4096, offs, 2, 0, p + 8192, 4096, None) == ls.OK
    assert L.labsort_merge_runs(p, p + 4096, offs, 2, 1, p + 8192, 4096, None) == ls.OK


def test_entries_that_accept_f32_check_their_arguments(ls):
    """Key type 2 passes the key-type check of the device sorts, the segmented sorts and top-k (the
    calls below fail on a later check: nothing is launched); 7 and -1 fail whatever else holds."""
    L = ls.lib
    buf, p = _buffers()
    BIG = 1 << 62
    TP = ls.segment_pair_tile_keys()
    # top-k: a NULL workspace, k > cols, on the three paths
    for rows, cols, k in ((4, 100, 7), (2, TP + 100, 9), (2, TP + 100, TP)):
        far = 1 << 40
        need = ls.topk_workspace_bytes(rows, cols, k)
        for largest in (0, 1):
            assert L.labsort_topk_device(far, rows, cols, k, largest, F32, 2 * far, None, None, need, None) == ls.ERR_ARG
            assert L.labsort_topk_device(far, rows, cols, k, largest, F32, 2 * far, None, 3 * far, need - 16, None) == ls.ERR_ARG
            assert L.labsort_topk_device(far, rows, cols, cols + 1, largest, F32, 2 * far, None, 3 * far, BIG, None) == ls.ERR_ARG
        for kt in (7, -1):
            assert L.labsort_topk_device(far, rows, cols, k, 0, kt, 2 * far, None, 3 * far, BIG, None) == ls.ERR_ARG
    assert L.labsort_topk_device(None, 0, 10, 5, 0, F32, None, None, None, 0, None) == ls.OK  # rows == 0
    # segmented sorts: workspace missing / short on both paths, keys and pairs
    for n, nseg, m in ((1000, 10, 100), (1000, 10, 0)):
        for pairs in (0, 1):
            need = L.labsort_segments_workspace_bytes(n, nseg, m, pairs)
            for ws, wsb in ((None, need), (p + 32768, need - 16)):
                if pairs:
                    st = L.labsort_sort_segments_pairs_device(p, p + 4096, p + 8192, p + 12288, n, p + 16384, nseg, m, F32,
                                                              ws, wsb, None)
                else:
                    st = L.labsort_sort_segments_device(p, p + 4096, n, p + 16384, nseg, m, F32, ws, wsb, None)
                assert st == ls.ERR_ARG
    for kt in (7, -1):
        assert L.labsort_sort_segments_device(p, p, 10, p, 1, 10, kt, p, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort_segments_pairs_device(p, p + 64, p, p + 64, 10, p, 1, 10, kt, p, BIG, None) == ls.ERR_ARG
    assert L.labsort_sort_segments_device(None, None, 0, None, 0, 0, F32, None, 0, None) == ls.OK  # n == 0
    # whole-array sorts: workspace missing / short; pairs aliased on one side only
    for n in (100, 1 << 17, 1 << 20):
        for algo in ("radix", "merge", "auto"):
            a = ls.ALGO[algo]
            need = ls.workspace_bytes(n, algo)
            assert L.labsort_sort_device(p, p, n, F32, a, None, need, None) == ls.ERR_ARG
            assert L.labsort_sort_device(p, p, n, F32, a, p, need - 16, None) == ls.ERR_ARG
            need = ls.pairs_workspace_bytes(n, algo)
            assert L.labsort_sort_pairs_device(p, p + 64, p, p + 64, n, F32, a, None, need, None) == ls.ERR_ARG
            assert L.labsort_sort_pairs_device(p, p + 64, p, p + 64, n, F32, a, p, need - 16, None) == ls.ERR_ARG
            assert L.labsort_sort_pairs_device(p, p + 64, p, p + 128, n, F32, a, p, BIG, None) == ls.ERR_ARG
            for kt in (7, -1):
                assert L.labsort_sort_device(p, p, n, kt, a, p, BIG, None) == ls.ERR_ARG
                assert L.labsort_sort_pairs_device(p, p + 64, p, p + 64, n, kt, a, p, BIG, None) == ls.ERR_ARG
    assert L.labsort_sort_device(None, None, 0, F32, 0, None, 0, None) == ls.OK  # n == 0


def test_workspace_sizes_unchanged(ls):
    """labsort_topk_workspace_bytes and labsort_segments_workspace_bytes take no key type: their values
    over the grids tests/test_topk_abi.py and tests/test_segsort_abi.py walk are those recorded at the
    commit before float32 keys (tests/golden/f32_workspace_sizes.json)."""
    g = json.load(open(GOLDEN))
    assert g["segment_tile_keys"] == ls.segment_tile_keys()
    assert g["segment_pair_tile_keys"] == ls.segment_pair_tile_keys()
    assert len(g["topk"]) > 200 and len(g["segments"]) > 1000
    for rows, cols, k, want in g["topk"]:
        assert ls.topk_workspace_bytes(rows, cols, k) == want, (rows, cols, k)
    for n, nseg, m, pairs, want in g["segments"]:
        assert ls.segments_workspace_bytes(n, nseg, m, bool(pairs)) == want, (n, nseg, m, pairs)
