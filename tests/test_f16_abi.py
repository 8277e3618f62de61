"""CPU tests of the 16-bit float key types (LABSORT_KEY_BF16 = 3, LABSORT_KEY_F16 = 4,
include/labsort.h): the order map the kernels compile, pinned for all 65536 words through
labsort_key_order_bits / labsort_key_from_order_bits against the numpy model (tests/f16_model.py);
top-k's argument checks with the new types; every other entry keeps rejecting them; ls.topk's
checks that come before the device.  No kernel is launched: every device entry called below
returns before its first launch."""
import ctypes
import os

import numpy as np
import pytest

import f16_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = {"bf16": 3, "f16": 4}
ALL = np.arange(1 << 16, dtype=np.uint32)
KINDS = pytest.mark.parametrize("kind", M.KINDS)


def lib_map(ls, words, kind, inverse=False):
    f = ls.lib.labsort_key_from_order_bits if inverse else ls.lib.labsort_key_order_bits
    return np.array([f(int(w), ls.KEY[kind]) for w in words], dtype=np.uint32)


def test_key_type_constants(ls):
    assert ls.KEY["bf16"] == 3 and ls.KEY["f16"] == 4
    assert (ls.KEY["u32"], ls.KEY["i32"], ls.KEY["f32"]) == (0, 1, 2)
    hdr = open(os.path.join(REPO, "include", "labsort.h")).read()
    assert "#define LABSORT_KEY_BF16 3" in hdr and "#define LABSORT_KEY_F16 4" in hdr


@KINDS
def test_order_map_exhaustive(ls, kind):
    """All 65536 words: the image is the model's, the inverse is unord16, every non-NaN word
    round-trips, every NaN maps to 0xFFFF and comes back as 0x7FFF (a NaN in both formats)."""
    x = ALL.astype(np.uint16)
    o = lib_map(ls, ALL, kind)
    np.testing.assert_array_equal(o, M.ord16(x, kind).astype(np.uint32))
    assert int(o.max()) == 0xFFFF
    back = lib_map(ls, ALL, kind, inverse=True)  # the inverse of every image value, NaN image included
    np.testing.assert_array_equal(back, M.unord16(x).astype(np.uint32))
    nan = M.is_nan16(x, kind)
    assert int(nan.sum()) == 2 * (0x7FFF - M.INF[kind])
    rt = back[o]  # unord16(ord16(x))
    np.testing.assert_array_equal(rt[~nan], ALL[~nan])
    assert np.all(o[nan] == 0xFFFF) and np.all(rt[nan] == 0x7FFF)
    assert M.is_nan16(np.uint16(0x7FFF), "bf16") and M.is_nan16(np.uint16(0x7FFF), "f16")
    # only the low 16 bits of the argument count
    hi = np.array([0x12340000, 0xFFFF0000, 0x00010000], dtype=np.uint32)
    for w in (0x0000, 0x8000, 0x3C00, 0xBF80, 0x7FC0, 0xFE01):
        for h in hi:
            assert ls.key_order_bits(int(h) | w, kind) == int(o[w])
            assert ls.key_from_order_bits(int(h) | w, kind) == int(back[w])


@KINDS
def test_order_map_is_the_float_order(ls, kind):
    """Over all non-NaN words: a strict float inequality implies a strict image inequality, equal
    floats differ in the image only as -0.0 / +0.0, and -0.0 sits exactly one below +0.0."""
    x = ALL.astype(np.uint16)
    ok = ~M.is_nan16(x, kind)
    w, o = x[ok], lib_map(ls, ALL, kind)[ok].astype(np.int64)
    f = M.as_float32(w, kind)
    assert not np.any(np.isnan(f))
    q = np.argsort(f, kind="stable")
    fs, os_ = f[q], o[q]
    strict = fs[:-1] < fs[1:]
    assert np.all(os_[:-1][strict] < os_[1:][strict])
    p = np.argsort(o, kind="stable")
    assert np.all(f[p][:-1] <= f[p][1:])
    assert len(np.unique(o)) == o.size  # distinct words, distinct images
    S = M.specials(kind)
    img = {k: ls.key_order_bits(v, kind) for k, v in S.items()}
    assert img["-0"] + 1 == img["+0"] == 0x8000
    assert (img["-inf"] < img["-max"] < img["-denorm_min"] < img["-0"] < img["+0"] < img["+denorm_min"] < img["+max"]
            < img["+inf"] < img["qnan"])
    assert img["qnan"] == img["-qnan1"] == img["snan"] == img["-snan"] == 0xFFFF


def test_other_key_types_unchanged(ls):
    for w in (0, 1, 0x7FC00000, 0x80000000, 0xFFFFFFFF, 0x12348000):
        assert ls.key_order_bits(w, "u32") == w and ls.key_from_order_bits(w, "u32") == w
        assert ls.key_order_bits(w, "i32") == w ^ 0x80000000
        assert ls.lib.labsort_key_order_bits(w, 7) == w and ls.lib.labsort_key_from_order_bits(w, 5) == w
    assert ls.key_order_bits(0x7FC00000, "f32") == 0xFFFFFFFF and ls.key_from_order_bits(0xFFFFFFFF, "f32") == 0x7FFFFFFF


def _buffers():
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += (-p) % 256
    return buf, p


@KINDS
def test_every_other_entry_rejects_the_type(ls, kind):
    """device_key_type_ok() and key_type_ok() stay as they were: the whole-array sorts, both
    segmented sorts, the host-pointer sort, the run merge and the bound query return ERR_ARG for key
    types 3 and 4 with arguments that are otherwise good; their empty calls return before the key
    type is looked at, as for every type (labsort_merge_runs looks at it first, as for float32)."""
    L, kt = ls.lib, KT[kind]
    buf, p = _buffers()
    BIG = 1 << 62
    for n in (100, 1 << 17, 1 << 20):
        for algo in ("radix", "merge", "auto"):
            a = ls.ALGO[algo]
            assert L.labsort_sort_device(p, p, n, kt, a, p, BIG, None) == ls.ERR_ARG
            assert L.labsort_sort_pairs_device(p, p + 64, p, p + 64, n, kt, a, p, BIG, None) == ls.ERR_ARG
    for m in (10, 0):
        assert L.labsort_sort_segments_device(p, p, 10, p, 1, m, kt, p, BIG, None) == ls.ERR_ARG
        assert L.labsort_sort_segments_pairs_device(p, p + 64, p, p + 64, 10, p, 1, m, kt, p, BIG, None) == ls.ERR_ARG
    assert L.labsort_sort_host(p, 100, kt, ls.ALGO["auto"]) == ls.ERR_ARG
    offs = (ctypes.c_size_t * 3)(0, 50, 100)
    assert L.labsort_merge_runs(p, p + 4096, offs, 2, kt, p + 8192, BIG, None) == ls.ERR_ARG
    assert L.labsort_upper_bound(p, 10, kt, p + 4096, 4, p + 8192, None) == ls.ERR_ARG
    # empty calls
    assert L.labsort_sort_device(None, None, 0, kt, 0, None, 0, None) == ls.OK
    assert L.labsort_sort_pairs_device(None, None, None, None, 0, kt, 0, None, 0, None) == ls.OK
    assert L.labsort_sort_segments_device(None, None, 0, None, 0, 0, kt, None, 0, None) == ls.OK
    assert L.labsort_sort_segments_pairs_device(None, None, None, None, 0, None, 0, 0, kt, None, 0, None) == ls.OK
    assert L.labsort_sort_host(None, 0, kt, ls.ALGO["auto"]) == ls.OK
    assert L.labsort_upper_bound(p, 10, kt, p + 4096, 0, p + 8192, None) == ls.OK
    empty = (ctypes.c_size_t * 3)(0, 0, 0)
    assert L.labsort_merge_runs(p, p + 4096, empty, 2, kt, p + 8192, 4096, None) == ls.ERR_ARG


@KINDS
def test_topk_argument_checks(ls, kind):
    """On the three paths (short rows, the select, whole-row sorting): NULL or short workspace,
    k > cols, an odd d_keys or d_keys_out address, an output that overlaps the input by its 2-byte
    extents; the same calls with the addresses apart pass every check before the workspace's."""
    L, kt = ls.lib, KT[kind]
    BIG = 1 << 62
    TP = ls.segment_pair_tile_keys()
    far = 1 << 40
    for rows, cols, k in ((4, 100, 7), (2, TP + 100, 9), (2, TP + 100, TP)):
        need = ls.topk_workspace_bytes(rows, cols, k)
        nin, nout = rows * cols * 2, rows * k * 2  # bytes of the 16-bit matrices
        for largest in (0, 1):
            def call(keys=far, out=2 * far, idx=None, ws=3 * far, wsb=BIG, kk=k):
                return L.labsort_topk_device(keys, rows, cols, kk, largest, kt, out, idx, ws, wsb, None)
            assert call(ws=None, wsb=need) == ls.ERR_ARG
            assert call(wsb=need - 16) == ls.ERR_ARG
            assert call(kk=cols + 1) == ls.ERR_ARG
            assert call(keys=far + 1) == ls.ERR_ARG
            assert call(out=2 * far + 1) == ls.ERR_ARG
            assert call(keys=far + 1, out=2 * far + 1) == ls.ERR_ARG
            # overlap by the real extents: the output's first byte on the input's last element, and
            # the output ending on the input's first element
            assert call(out=far + nin - 2) == ls.ERR_ARG
            assert call(out=far - nout + 2) == ls.ERR_ARG
            assert call(out=far) == ls.ERR_ARG
            assert call(idx=far + nin - 4) == ls.ERR_ARG
            assert call(idx=2 * far) == ls.ERR_ARG  # d_idx_out == d_keys_out
            # (an output directly behind the input, which 4-byte extents would reject, is accepted:
            # tests/test_gpu_f16_topk.py::test_output_directly_behind_the_input)
    assert L.labsort_topk_device(None, 0, 10, 5, 0, kt, None, None, None, 0, None) == ls.OK  # rows == 0
    assert L.labsort_topk_device(far + 1, 0, 10, 5, 1, kt, far + 3, None, None, 0, None) == ls.OK
    # the workspace size takes no key type: a 16-bit call needs what a 32-bit one does
    assert ls.topk_workspace_bytes(2, TP + 100, 9) == ls.lib.labsort_topk_workspace_bytes(2, TP + 100, 9)


def test_topk_rejects_other_inputs_before_the_device(ls):
    """ls.topk: TypeError for a dtype that is no key type and for a non-contiguous tensor, on CPU
    tensors, so before any device call."""
    import torch
    for dt in (torch.float64, torch.int64, torch.int16, torch.uint8):
        with pytest.raises(TypeError):
            ls.topk(torch.zeros((4, 8), dtype=dt), 2)
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.int32):
        with pytest.raises(TypeError):
            ls.topk(torch.zeros((8, 4), dtype=dt).t(), 2)
        with pytest.raises(TypeError):
            ls.topk(torch.zeros((2, 4, 8), dtype=dt), 2)
    with pytest.raises(TypeError):
        ls.topk(np.zeros((4, 8), dtype=np.float32), 2)
