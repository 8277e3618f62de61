"""labsort -- MI355X-native (gfx950) integer sort behind the reference's order_array API.

The product is the native library `liblabsort.so` (HIP kernels + C++ host
orchestration, C-ABI in include/labsort.h).  This module is a thin ctypes view of
it for Python callers, tests and bench.py:

  order_array(a)          lab.h:9 / lab.cu:303  -- int32 numpy array sorted in place
                          through the GPU (host pointer, synchronous)
  order_with_trust(a)     lab.h:10 / lab.cu:404 -- thrust::sort on the host pointer
  sort_device(...)        the device-pointer sort (keys already in HBM)
  wave_tile_sort, tile_sort, merge_pass, merge, histogram  -- the building blocks

There is no CPU fallback: if the shared library is missing this module raises
at import, and every device call raises LabsortError on a failed status.
The package directory name is not a Python identifier; import it with
``importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# LABSORT_LIBRARY: path of an alternative build (diagnostic builds under harness/exp)
LIB_PATH = os.environ.get("LABSORT_LIBRARY") or os.path.join(HERE, "liblabsort.so")

OK, ERR_ARG, ERR_HIP, ERR_DEVICE, ERR_PEER = 0, 1, 2, 3, 4
ALGO = {"radix": 0, "merge": 1, "radix1": 2, "auto": 3}
# "f32": IEEE-754 order with -0.0 < +0.0 and every NaN equal and last; the device sorts, the segmented
# sorts and top-k take it, the host-pointer and multi-GPU entries do not (labsort.h)
# "bf16", "f16": 16-bit elements, the same order at 16 bits; top-k, the row sort and sort16 alone take them
# "u64", "i64", "f64": 8-byte elements, sort64 alone takes them (5 to 7 are not assigned)
KEY = {"u32": 0, "i32": 1, "f32": 2, "bf16": 3, "f16": 4, "u64": 8, "i64": 9, "f64": 10}
DIST = {"u32": 0, "u31": 1, "mod100": 2, "mod1000": 3, "sorted": 4, "reversed": 5, "const": 6, "lowbits": 7}
KCLASS = {"histogram": 0, "onesweep": 1, "tile_sort": 2, "merge": 3, "partition": 4, "gsweep": 5, "gcopy": 6,
          "copy": 7, "merge4": 8, "segsort": 9, "topk": 10}
# topk_device sorts whole rows from k > cols // TOPK_SORT_DIV (LABSORT_TOPK_SORT_DIV in labsort.h)
TOPK_SORT_DIV = 4

# exported symbols of include/labsort.h + lab.h (checked by tests/test_abi.py)
C_SYMBOLS = [
    "labsort_version", "labsort_error_string", "labsort_last_hip_error", "labsort_hip_error_string",
    "labsort_max_keys", "labsort_tile_keys", "labsort_merge_tile_keys", "labsort_workspace_bytes",
    "labsort_sort_device", "labsort_sort_host", "labsort_wave_tile_sort", "labsort_tile_sort",
    "labsort_merge_parts", "labsort_merge_pass", "labsort_merge", "labsort_histogram", "labsort_fill",
    "labsort_count_descents", "labsort_timing_enable", "labsort_timing_read", "labsort_upper_bound", "sort",
    "labsort_merge_runs_workspace_bytes", "labsort_merge_runs",
    "labsort_pair_tile_keys", "labsort_pairs_workspace_bytes", "labsort_sort_pairs_device",
    "labsort_workspace_status", "labsort_pairs_workspace_status", "labsort_radix_path",
    "labsort_radix_counting",
    "labsort_sort_host_multi", "labsort_sort_host_ranks", "labsort_multi_timing", "labsort_multi_last_hip_error",
    "labsort_multi_plan", "labsort_multi_error_detail", "labsort_multi_range_counts",
    "labsort_comm_unique_id", "labsort_comm_init_rccl", "labsort_comm_init_host", "labsort_comm_destroy",
    "labsort_dist_sort", "labsort_dist_timing", "labsort_dist_last_hip_error",
    "labsort_multi_collectives", "labsort_dist_collectives", "labsort_copy",
    "labsort_comm_set_timeout", "labsort_test_fault",
    "labsort_segment_tile_keys", "labsort_segment_pair_tile_keys", "labsort_segment_class_edges",
    "labsort_segments_workspace_bytes", "labsort_sort_segments_device", "labsort_sort_segments_pairs_device",
    "labsort_segments_workspace_status",
    "labsort_topk_workspace_bytes", "labsort_topk_device", "labsort_topk_workspace_status",
    "labsort_sort_rows_workspace_bytes", "labsort_sort_rows_device", "labsort_sort_rows_workspace_status",
    "labsort_sort16_chunk_keys", "labsort_sort16_workspace_bytes", "labsort_sort16_device",
    "labsort_sort16_workspace_status",
    "labsort_sort64_chunk_keys", "labsort_sort64_workspace_bytes", "labsort_sort64_device",
    "labsort_sort64_workspace_status", "labsort_sort64_passes",
    "labsort_key_order_bits64", "labsort_key_from_order_bits64",
    "labsort_kth_row_keys", "labsort_kth_workspace_bytes", "labsort_kth_device", "labsort_kth_workspace_status",
    "labsort_topk_mask_workspace_bytes", "labsort_topk_mask_device", "labsort_topk_mask_workspace_status",
    "labsort_top_p_weight", "labsort_top_p_workspace_bytes", "labsort_top_p_device", "labsort_top_p_workspace_status",
    "labsort_sample_workspace_bytes", "labsort_sample_device", "labsort_sample_workspace_status",
    "labsort_key_order_bits", "labsort_key_from_order_bits",
    "labsort_unique_chunk_keys", "labsort_unique_workspace_bytes", "labsort_unique_device",
    "labsort_unique_workspace_status",
    "labsort_searchsorted_row_keys", "labsort_searchsorted_chunk_values", "labsort_searchsorted_workspace_bytes",
    "labsort_searchsorted_device",
    "labsort_bucket_counts_row_edges", "labsort_bucket_counts_workspace_bytes", "labsort_bucket_counts_device",
    "labsort_bincount_row_bins", "labsort_bincount_device",
]
UNIQUE_CONSECUTIVE = 1  # LABSORT_UNIQUE_CONSECUTIVE
XFER = {"auto": 0, "rccl": 1, "peer": 2}
MULTI_PHASES = ["h2d", "local_sort", "plan", "exchange", "merge", "d2h", "total", "plan_work", "plan_wait"]
COLLECTIVES = ["samples", "counts", "grow"]  # the schedule's collectives, in order (labsort.h)
CXX_SYMBOLS = ["_Z11order_arrayPii", "_Z16order_with_trustPii"]


class LabsortError(RuntimeError):
    """A failed LABSORT_* status; .status holds the code (ERR_ARG, ERR_HIP, ERR_DEVICE,
    ERR_PEER)."""

    def __init__(self, msg: str, status: int = 0):
        super().__init__(msg)
        self.status = status


# labsort_host_coll (include/labsort.h): host collectives supplied by the caller
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                                ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t))


class HostColl(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("allgather", ALLGATHER_FN), ("alltoallv", ALLTOALLV_FN)]


def host_coll(obj) -> HostColl:
    """labsort_host_coll whose callbacks call obj.allgather(h_in, h_out, nbytes) and
    obj.alltoallv(h_send, send_bytes, h_recv, recv_bytes) (raw host addresses and lists
    of byte counts).  A Python exception in a callback becomes a failed status.  Keep
    the returned structure alive while the communicator uses it."""
    import traceback

    def ag(_ctx, h_in, h_out, nbytes):
        try:
            obj.allgather(h_in, h_out, int(nbytes))
            return 0
        except Exception:
            traceback.print_exc()
            return 1

    def a2a(_ctx, h_send, sb, h_recv, rb):
        try:
            n = obj.world
            obj.alltoallv(h_send, [int(sb[i]) for i in range(n)], h_recv, [int(rb[i]) for i in range(n)])
            return 0
        except Exception:
            traceback.print_exc()
            return 1

    return HostColl(None, ALLGATHER_FN(ag), ALLTOALLV_FN(a2a))


def _load() -> ctypes.CDLL:
    # One HIP runtime per process: torch ships its own libamdhip64.so (SONAME
    # libamdhip64.so.7).  Loading torch first makes liblabsort's DT_NEEDED
    # libamdhip64.so.7 bind to that already-loaded runtime, so torch tensors and
    # our kernels share one device context.  Loaded the other way round, a second
    # runtime would come up and find no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the labsort path has no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    p, sz, i, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    L.labsort_version.restype = ctypes.c_char_p
    L.labsort_error_string.restype = ctypes.c_char_p
    L.labsort_error_string.argtypes = [i]
    L.labsort_hip_error_string.restype = ctypes.c_char_p
    L.labsort_hip_error_string.argtypes = [i]
    for f in ("labsort_max_keys", "labsort_workspace_bytes"):
        getattr(L, f).restype = sz
    L.labsort_max_keys.argtypes = [i]
    L.labsort_tile_keys.restype = sz
    L.labsort_merge_tile_keys.restype = sz
    L.labsort_merge_parts.restype = sz
    L.labsort_merge_parts.argtypes = [sz]
    L.labsort_workspace_bytes.argtypes = [sz, i]
    L.labsort_sort_device.argtypes = [p, p, sz, i, i, p, sz, p]
    L.labsort_sort_host.argtypes = [p, sz, i, i]
    L.labsort_wave_tile_sort.argtypes = [p, sz, i, p]
    L.labsort_tile_sort.argtypes = [p, p, sz, i, p]
    L.labsort_merge_pass.argtypes = [p, p, sz, sz, i, p, p]
    L.labsort_merge.argtypes = [p, sz, p, sz, p, sz, sz, i, p, p]
    L.labsort_merge_runs_workspace_bytes.restype = sz
    L.labsort_merge_runs_workspace_bytes.argtypes = [sz]
    L.labsort_merge_runs.argtypes = [p, p, ctypes.POINTER(sz), i, i, p, sz, p]
    L.labsort_pair_tile_keys.restype = sz
    L.labsort_pair_tile_keys.argtypes = []
    L.labsort_pairs_workspace_bytes.restype = sz
    L.labsort_pairs_workspace_bytes.argtypes = [sz, i]
    L.labsort_sort_pairs_device.argtypes = [p, p, p, p, sz, i, i, p, sz, p]
    L.labsort_workspace_status.argtypes = [p, sz, i, p]
    if hasattr(L, "labsort_radix_path"):  # (an older build loaded through LABSORT_LIBRARY for an A/B has none)
        L.labsort_radix_path.argtypes = [p, sz, p]
    if hasattr(L, "labsort_radix_counting"):  # (as labsort_radix_path above)
        L.labsort_radix_counting.argtypes = [p, sz, p]
    L.labsort_sort_host_multi.argtypes = [p, sz, i, i]
    L.labsort_sort_host_ranks.argtypes = [p, sz, i, i, p, i]
    L.labsort_multi_timing.argtypes = [ctypes.POINTER(ctypes.c_double), i, ctypes.POINTER(sz)]
    L.labsort_multi_plan.argtypes = [ctypes.POINTER(p), ctypes.POINTER(sz), i, i, ctypes.POINTER(sz)]
    L.labsort_multi_range_counts.argtypes = [ctypes.POINTER(sz), i]
    L.labsort_multi_error_detail.restype = ctypes.c_char_p
    L.labsort_multi_error_detail.argtypes = []
    L.labsort_comm_unique_id.argtypes = [p]
    L.labsort_comm_init_rccl.argtypes = [ctypes.POINTER(p), p, i, i]
    L.labsort_comm_init_host.argtypes = [ctypes.POINTER(p), i, i, ctypes.POINTER(HostColl)]
    L.labsort_comm_destroy.argtypes = [p]
    L.labsort_comm_set_timeout.argtypes = [p, ctypes.c_double]
    L.labsort_test_fault.argtypes = [ctypes.c_char_p, i]
    L.labsort_dist_sort.argtypes = [p, p, sz, i, p, ctypes.POINTER(p), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.labsort_dist_timing.argtypes = [p, ctypes.POINTER(ctypes.c_double), i, ctypes.POINTER(sz)]
    L.labsort_dist_last_hip_error.argtypes = [p]
    L.labsort_multi_collectives.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), i, i]
    L.labsort_dist_collectives.argtypes = [p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), i]
    L.labsort_copy.argtypes = [p, p, sz, p]
    L.labsort_pairs_workspace_status.argtypes = [p, sz, i, p]
    L.labsort_segment_tile_keys.restype = sz
    L.labsort_segment_tile_keys.argtypes = []
    L.labsort_segment_pair_tile_keys.restype = sz
    L.labsort_segment_pair_tile_keys.argtypes = []
    L.labsort_segment_class_edges.argtypes = [i, ctypes.POINTER(sz), i]
    L.labsort_segments_workspace_bytes.restype = sz
    L.labsort_segments_workspace_bytes.argtypes = [sz, sz, sz, i]
    L.labsort_sort_segments_device.argtypes = [p, p, sz, p, sz, sz, i, p, sz, p]
    L.labsort_sort_segments_pairs_device.argtypes = [p, p, p, p, sz, p, sz, sz, i, p, sz, p]
    L.labsort_segments_workspace_status.argtypes = [p, p]
    L.labsort_topk_workspace_bytes.restype = sz
    L.labsort_topk_workspace_bytes.argtypes = [sz, sz, sz]
    L.labsort_topk_device.argtypes = [p, sz, sz, sz, i, i, p, p, p, sz, p]
    L.labsort_topk_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_sort_rows_device"):  # (as labsort_radix_path above)
        L.labsort_sort_rows_workspace_bytes.restype = sz
        L.labsort_sort_rows_workspace_bytes.argtypes = [sz, sz]
        L.labsort_sort_rows_device.argtypes = [p, sz, sz, i, i, p, p, p, sz, p]
        L.labsort_sort_rows_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_sort16_device"):  # (as labsort_radix_path above)
        L.labsort_sort16_chunk_keys.restype = sz
        L.labsort_sort16_chunk_keys.argtypes = []
        L.labsort_sort16_workspace_bytes.restype = sz
        L.labsort_sort16_workspace_bytes.argtypes = [sz, sz, i]
        L.labsort_sort16_device.argtypes = [p, sz, sz, i, i, p, p, p, sz, p]
        L.labsort_sort16_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_sort64_device"):  # (as labsort_radix_path above)
        L.labsort_sort64_chunk_keys.restype = sz
        L.labsort_sort64_chunk_keys.argtypes = []
        L.labsort_sort64_workspace_bytes.restype = sz
        L.labsort_sort64_workspace_bytes.argtypes = [sz, sz, i]
        L.labsort_sort64_device.argtypes = [p, sz, sz, i, i, p, p, p, sz, p]
        L.labsort_sort64_workspace_status.argtypes = [p, p]
        L.labsort_sort64_passes.argtypes = [p, p]
        for f in ("labsort_key_order_bits64", "labsort_key_from_order_bits64"):
            getattr(L, f).restype = u64
            getattr(L, f).argtypes = [u64, i]
    if hasattr(L, "labsort_kth_device"):  # (as labsort_radix_path above)
        L.labsort_kth_row_keys.restype = sz
        L.labsort_kth_row_keys.argtypes = []
        L.labsort_kth_workspace_bytes.restype = sz
        L.labsort_kth_workspace_bytes.argtypes = [sz, sz]
        L.labsort_kth_device.argtypes = [p, sz, sz, sz, p, i, i, p, p, p, sz, p]
        L.labsort_kth_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_topk_mask_device"):  # (as labsort_radix_path above)
        L.labsort_topk_mask_workspace_bytes.restype = sz
        L.labsort_topk_mask_workspace_bytes.argtypes = [sz, sz]
        L.labsort_topk_mask_device.argtypes = [p, sz, sz, sz, p, i, i, ctypes.c_uint32, p, p, p, sz, p]
        L.labsort_topk_mask_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_top_p_device"):  # (as labsort_radix_path above)
        L.labsort_top_p_weight.restype = u64
        L.labsort_top_p_weight.argtypes = [ctypes.c_uint32, i]
        L.labsort_top_p_workspace_bytes.restype = sz
        L.labsort_top_p_workspace_bytes.argtypes = [sz, sz]
        L.labsort_top_p_device.argtypes = [p, sz, sz, ctypes.c_float, p, i, ctypes.c_uint32, p, p, p, p, sz, p]
        L.labsort_top_p_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_sample_device"):  # (as labsort_radix_path above)
        L.labsort_sample_workspace_bytes.restype = sz
        L.labsort_sample_workspace_bytes.argtypes = [sz, sz, sz]
        L.labsort_sample_device.argtypes = [p, sz, sz, p, sz, i, p, p, sz, p]
        L.labsort_sample_workspace_status.argtypes = [p, p]
    if hasattr(L, "labsort_unique_device"):  # (as labsort_radix_path above)
        L.labsort_unique_chunk_keys.restype = sz
        L.labsort_unique_chunk_keys.argtypes = []
        L.labsort_unique_workspace_bytes.restype = sz
        L.labsort_unique_workspace_bytes.argtypes = [sz, i, i, i]
        L.labsort_unique_device.argtypes = [p, sz, i, i, p, p, p, p, p, p, sz, p]
        L.labsort_unique_workspace_status.argtypes = [p, sz, i, i, p]
    if hasattr(L, "labsort_searchsorted_device"):  # (as labsort_radix_path above)
        L.labsort_searchsorted_row_keys.restype = sz
        L.labsort_searchsorted_row_keys.argtypes = [i]
        L.labsort_searchsorted_chunk_values.restype = sz
        L.labsort_searchsorted_chunk_values.argtypes = []
        L.labsort_searchsorted_workspace_bytes.restype = sz
        L.labsort_searchsorted_workspace_bytes.argtypes = [sz, sz, i]
        L.labsort_searchsorted_device.argtypes = [p, sz, sz, p, p, sz, sz, i, i, p, p, sz, p]
    if hasattr(L, "labsort_bucket_counts_device"):  # (as labsort_radix_path above)
        L.labsort_bucket_counts_row_edges.restype = sz
        L.labsort_bucket_counts_row_edges.argtypes = [i]
        L.labsort_bucket_counts_workspace_bytes.restype = sz
        L.labsort_bucket_counts_workspace_bytes.argtypes = [sz, sz, i]
        L.labsort_bucket_counts_device.argtypes = [p, sz, sz, p, sz, sz, i, i, p, p, sz, p]
        L.labsort_bincount_row_bins.restype = sz
        L.labsort_bincount_row_bins.argtypes = []
        L.labsort_bincount_device.argtypes = [p, sz, sz, sz, i, p, p]
    if hasattr(L, "labsort_key_order_bits"):  # (as labsort_radix_path above)
        for f in ("labsort_key_order_bits", "labsort_key_from_order_bits"):
            getattr(L, f).restype = ctypes.c_uint32
            getattr(L, f).argtypes = [ctypes.c_uint32, i]
    L.labsort_histogram.argtypes = [p, sz, i, i, p, p]
    L.labsort_fill.argtypes = [p, sz, u64, i, u64, u64, p]
    L.labsort_count_descents.argtypes = [p, sz, i, p, p]
    L.labsort_upper_bound.argtypes = [p, sz, i, p, sz, p, p]
    L.labsort_timing_enable.argtypes = [i]
    L.labsort_timing_read.argtypes = [i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]
    L.sort.argtypes = [p, i]
    L.sort.restype = None
    fn = getattr(L, "_Z11order_arrayPii")
    fn.argtypes = [p, i]
    fn.restype = None
    fn = getattr(L, "_Z16order_with_trustPii")
    fn.argtypes = [p, i]
    fn.restype = None
    return L


lib = _load()


def version() -> str:
    return lib.labsort_version().decode()


def _check(status: int, what: str) -> None:
    if status != OK:
        msg = lib.labsort_error_string(status).decode()
        if status == ERR_HIP:
            msg += ": " + lib.labsort_hip_error_string(lib.labsort_last_hip_error()).decode()
        raise LabsortError(f"{what} failed: {msg}", status)


def _ptr(x) -> int:
    """Device or host address of a torch tensor / numpy array / int."""
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    assert x.is_contiguous()
    return x.data_ptr()


def _stream(stream) -> int | None:
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


# ---- host-pointer drop-ins (lab.h) -------------------------------------------------
def order_array(a: np.ndarray) -> None:
    """Sort an int32 numpy array in place on the GPU (lab.cu:303 semantics).

    Unlike the C++ drop-in, which prints GPUassert and exits, this raises."""
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    _check(lib.labsort_sort_host(a.ctypes.data, a.size, KEY["i32"], _default_algo()), "order_array")


def sort_host(a: np.ndarray, algo: str = "radix") -> None:
    """Sort a uint32 or int32 numpy array in place through the GPU."""
    key = "i32" if a.dtype == np.int32 else "u32"
    assert a.dtype in (np.int32, np.uint32) and a.flags["C_CONTIGUOUS"]
    _check(lib.labsort_sort_host(a.ctypes.data, a.size, KEY[key], ALGO[algo]), "sort_host")


def order_with_trust(a: np.ndarray) -> None:
    """thrust::sort on the host pointer (lab.cu:404): rocThrust's sequential CPU sort."""
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    getattr(lib, "_Z16order_with_trustPii")(a.ctypes.data, a.size)


def _check_multi(status: int, what: str) -> None:
    if status != OK:
        detail = lib.labsort_multi_error_detail().decode()
        raise LabsortError(f"{what} failed: {lib.labsort_error_string(status).decode()}"
                           + (f" ({detail})" if detail else ""), status)


def sort_host_multi(a: np.ndarray, ngpus: int) -> None:
    """Sort a uint32/int32 numpy array in place across devices 0..ngpus-1 of this
    process (labsort_sort_host_multi: per-GPU shards, RCCL splitter exchange)."""
    key = "i32" if a.dtype == np.int32 else "u32"
    assert a.dtype in (np.int32, np.uint32) and a.flags["C_CONTIGUOUS"]
    _check_multi(lib.labsort_sort_host_multi(a.ctypes.data, a.size, KEY[key], ngpus), "sort_host_multi")


def sort_host_ranks(a: np.ndarray, devices, transport: str = "auto") -> None:
    """As sort_host_multi with an explicit rank -> device map (ranks may share a
    device with transport "peer": the whole schedule on one GPU)."""
    key = "i32" if a.dtype == np.int32 else "u32"
    assert a.dtype in (np.int32, np.uint32) and a.flags["C_CONTIGUOUS"]
    dv = (ctypes.c_int * len(devices))(*devices)
    _check_multi(lib.labsort_sort_host_ranks(a.ctypes.data, a.size, KEY[key], len(devices), dv, XFER[transport]),
                 "sort_host_ranks")


def multi_timing() -> tuple[dict, int]:
    """Phase times (ms) of the last multi-GPU host sort and the most key bytes one
    rank sent to its peers."""
    ms = (ctypes.c_double * len(MULTI_PHASES))()
    sent = ctypes.c_size_t(0)
    _check(lib.labsort_multi_timing(ms, len(MULTI_PHASES), ctypes.byref(sent)), "multi_timing")
    return dict(zip(MULTI_PHASES, list(ms))), sent.value


def multi_collectives(nranks: int) -> list:
    """Per rank of the last multi-GPU host sort: {collective: (arrive_ms, leave_ms)} on the
    host clock since that rank's start (-1: the collective did not run)."""
    k = len(COLLECTIVES)
    a, b = (ctypes.c_double * (nranks * k))(), (ctypes.c_double * (nranks * k))()
    _check(lib.labsort_multi_collectives(a, b, nranks, k), "multi_collectives")
    return [{COLLECTIVES[c]: (a[r * k + c], b[r * k + c]) for c in range(k)} for r in range(nranks)]


def multi_range_counts(nranks: int) -> list:
    """Keys of each rank's range of the sorted array in the last multi-GPU host sort."""
    c = (ctypes.c_size_t * nranks)()
    _check(lib.labsort_multi_range_counts(c, nranks), "multi_range_counts")
    return list(c)


def multi_plan(shards, key: str = "u32") -> np.ndarray:
    """Cut points of the multi-GPU exchange plan for sorted host shards (test hook):
    cuts[r, j] = first position of the piece rank r sends to rank j (cuts[r, p] = m_r)."""
    arrs = [np.ascontiguousarray(x).view(np.uint32) for x in shards]
    p = len(arrs)
    ptrs = (ctypes.c_void_p * p)(*[x.ctypes.data if x.size else None for x in arrs])
    ms = (ctypes.c_size_t * p)(*[x.size for x in arrs])
    cuts = (ctypes.c_size_t * (p * (p + 1)))()
    _check(lib.labsort_multi_plan(ptrs, ms, p, KEY[key], cuts), "multi_plan")
    return np.array(list(cuts), dtype=np.int64).reshape(p, p + 1)


def test_fault(phase: str | None, rank: int = -1) -> None:
    """TEST HOOK (labsort_test_fault): rank `rank` of the following multi-GPU sorts of this
    process fails at `phase` ("local_sort", "bounds", "recv", "grow", "exchange"); None
    disarms.  The product never arms it."""
    _check(lib.labsort_test_fault(phase.encode() if phase else None, rank), "test_fault")


def set_comm_timeout(seconds: float) -> None:
    """Deadline of every wait on the peers of the in-process RCCL transport and of the
    communicators created afterwards (labsort_comm_set_timeout(NULL, seconds))."""
    _check(lib.labsort_comm_set_timeout(None, float(seconds)), "comm_set_timeout")


class DistComm:
    """One rank's communicator of the distributed merge sort (labsort_comm_t; one
    process per GPU).  DistComm.rccl(world, rank, uid) over RCCL (uid from
    DistComm.unique_id() on rank 0, broadcast by the caller), or DistComm.host(world,
    rank, coll) over host collectives (an object with world, allgather and alltoallv:
    dist.GlooColl), which lets several ranks share one GPU in the tests."""

    def __init__(self, handle, keep=None):
        self.h = ctypes.c_void_p(handle)
        self._keep = keep

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _check_multi(lib.labsort_comm_unique_id(buf), "labsort_comm_unique_id")
        return buf.raw

    @classmethod
    def rccl(cls, world: int, rank: int, uid: bytes) -> "DistComm":
        h = ctypes.c_void_p(0)
        ub = ctypes.create_string_buffer(bytes(uid), 128)
        _check_multi(lib.labsort_comm_init_rccl(ctypes.byref(h), ub, world, rank), "labsort_comm_init_rccl")
        return cls(h.value)

    @classmethod
    def host(cls, world: int, rank: int, coll_obj) -> "DistComm":
        coll = host_coll(coll_obj)
        h = ctypes.c_void_p(0)
        _check_multi(lib.labsort_comm_init_host(ctypes.byref(h), world, rank, ctypes.byref(coll)),
                     "labsort_comm_init_host")
        return cls(h.value, keep=(coll, coll_obj))

    def sort(self, d_keys, m: int, key: str = "u32", stream=None) -> tuple[int, int, int]:
        """labsort_dist_sort: (device address, count, global offset) of this rank's range
        of the sorted array, valid until the next sort on this communicator."""
        res, cnt, goff = ctypes.c_void_p(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        st = lib.labsort_dist_sort(self.h, _ptr(d_keys) if m else None, m, KEY[key], _stream(stream),
                                   ctypes.byref(res), ctypes.byref(cnt), ctypes.byref(goff))
        _check_multi(st, "labsort_dist_sort")
        return res.value or 0, cnt.value, goff.value

    def sort_tensor(self, d_keys, m: int, key: str = "u32", stream=None, copy: bool = True):
        """As sort(), with the range as an int32 torch tensor and its global offset.  By
        default the range is copied out of the communicator's buffer; copy=False returns a
        zero-copy view of that buffer instead, which keeps this communicator alive but is
        INVALID after its next sort: that sort may overwrite the buffer, or free it and
        allocate a larger one (a range that outgrew it), leaving the view on freed memory."""
        ptr, cnt, goff = self.sort(d_keys, m, key, stream)
        v = self.view(ptr, cnt, owner=self)
        return (v.clone() if copy else v), goff

    @staticmethod
    def view(ptr: int, count: int, owner=None):
        """int32 torch tensor on the current device viewing `count` keys at device
        address `ptr` (__cuda_array_interface__; no copy).  `owner` (e.g. the DistComm whose
        buffer it is) is kept alive as long as the tensor."""
        import torch
        if count == 0:
            return torch.empty(0, dtype=torch.int32, device="cuda")

        class _View:
            __cuda_array_interface__ = {"shape": (count,), "typestr": "<i4", "data": (ptr, False), "version": 2,
                                        "strides": None}
        holder = _View()
        holder.owner = owner
        t = torch.as_tensor(holder, device="cuda")
        t._labsort_owner = holder  # the buffer's owner lives as long as the tensor
        return t

    def set_timeout(self, seconds: float) -> None:
        """Deadline of this communicator's waits on its peers (RCCL; labsort_comm_set_timeout)."""
        _check(lib.labsort_comm_set_timeout(self.h, float(seconds)), "comm_set_timeout")

    def timing(self) -> tuple[dict, int]:
        ms = (ctypes.c_double * len(MULTI_PHASES))()
        sent = ctypes.c_size_t(0)
        _check(lib.labsort_dist_timing(self.h, ms, len(MULTI_PHASES), ctypes.byref(sent)), "dist_timing")
        return dict(zip(MULTI_PHASES, list(ms))), sent.value

    def collectives(self) -> dict:
        """{collective: (arrive_ms, leave_ms)} of this rank's last sort (-1: not run)."""
        k = len(COLLECTIVES)
        a, b = (ctypes.c_double * k)(), (ctypes.c_double * k)()
        _check(lib.labsort_dist_collectives(self.h, a, b, k), "dist_collectives")
        return {COLLECTIVES[c]: (a[c], b[c]) for c in range(k)}

    def close(self) -> None:
        if self.h.value:
            _check_multi(lib.labsort_comm_destroy(self.h), "labsort_comm_destroy")
            self.h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            if self.h.value:
                lib.labsort_comm_destroy(self.h)
        except Exception:
            pass


def _default_algo() -> int:
    """as the C++ drop-ins: LABSORT_ALGO names the algorithm, else "auto" (merge up to
    LABSORT_AUTO_MERGE_MAX_KEYS keys, radix above)"""
    return ALGO.get(os.environ.get("LABSORT_ALGO", "auto"), ALGO["auto"])


# ---- device API (torch tensors or raw device addresses) ----------------------------
def workspace_bytes(n: int, algo: str = "radix") -> int:
    return int(lib.labsort_workspace_bytes(n, ALGO[algo]))


GS_MIN_N, GS_MAX_N = 1 << 16, 1 << 25  # LABSORT_ALGO_RADIX's gathered-pass window (common.h)


def radix_impl(n: int) -> str:
    """Which LSD implementation LABSORT_ALGO_RADIX runs for n keys: "gather" (gsweep.hip)
    or "onesweep" (kernels.hip), as api.hip's use_gather decides."""
    env = os.environ.get("LABSORT_RADIX_IMPL", "")
    if env == "gather":
        return "gather"
    if GS_MIN_N <= n < GS_MAX_N and env != "onesweep":
        return "gather"
    return "onesweep"


def max_keys(algo: str = "radix") -> int:
    return int(lib.labsort_max_keys(ALGO[algo]))


def tile_keys() -> int:
    return int(lib.labsort_tile_keys())


def merge_tile_keys() -> int:
    return int(lib.labsort_merge_tile_keys())


def merge_parts(n: int) -> int:
    return int(lib.labsort_merge_parts(n))


def _workspace(workspace, nbytes):
    """(workspace, its size in bytes, own) for a device call.  Without a caller-owned workspace
    (own), max(nbytes(), 1) bytes are allocated, and the caller synchronises and checks the
    status itself.  A raw device address counts as nbytes() long."""
    own = workspace is None
    if own:
        import torch
        workspace = torch.empty(max(nbytes(), 1), dtype=torch.uint8, device="cuda")
    wsb = workspace.numel() * workspace.element_size() if hasattr(workspace, "numel") else nbytes()
    return workspace, wsb, own


def sort_device(d_in, d_out, n: int, key: str = "u32", algo: str = "radix", workspace=None,
                workspace_bytes_: int | None = None, stream=None) -> None:
    """Sort n keys d_in -> d_out (may alias) asynchronously on `stream`.  key: "u32", "i32" or
    "f32" (float32 tensors as they are: IEEE-754 order, -0.0 < +0.0, NaNs equal and last).

    With a caller-owned `workspace` the call stays asynchronous; check the kernels'
    own error report with workspace_status() once the result is needed.  Without
    one, the call allocates a workspace, synchronises and checks it itself."""
    workspace, wsb, own = _workspace(workspace, lambda: workspace_bytes(n, algo))
    if workspace_bytes_ is not None:
        wsb = workspace_bytes_
    _check(lib.labsort_sort_device(_ptr(d_in), _ptr(d_out), n, KEY[key], ALGO[algo], _ptr(workspace), wsb,
                                   _stream(stream)), "sort_device")
    if own:
        workspace_status(workspace, n, algo, stream)


def workspace_status(workspace, n: int, algo: str = "radix", stream=None) -> None:
    """Synchronise `stream` and raise LabsortError(device-side error) if a kernel of the
    last sort_device(n, algo) on `workspace` reported a failure (labsort_workspace_status)."""
    _check(lib.labsort_workspace_status(_ptr(workspace), n, ALGO[algo], _stream(stream)), "sort_device (status)")


def radix_path(workspace, n: int, stream=None) -> int:
    """Synchronise `stream`; 1 if the last keys-only radix sort of n keys on `workspace` took the
    hybrid path (two scatter passes, buckets finished in LDS), 0 for the classic passes."""
    r = int(lib.labsort_radix_path(_ptr(workspace), n, _stream(stream)))
    if r < 0:
        _check(-r, "radix_path")
    return r


def radix_counting(workspace, n: int, stream=None) -> int:
    """Synchronise `stream`; which upfront count the last keys-only radix sort of n keys on
    `workspace` ran: 0 the full count only, 1 the hybrid path's lean count only, 2 the lean count
    and then the full one (labsort_radix_counting)."""
    r = int(lib.labsort_radix_counting(_ptr(workspace), n, _stream(stream)))
    if r < 0:
        _check(-r, "radix_counting")
    return r


def pairs_workspace_status(workspace, n: int, algo: str = "radix", stream=None) -> None:
    """As workspace_status, for the last sort_pairs_device(n, algo) on `workspace`."""
    _check(lib.labsort_pairs_workspace_status(_ptr(workspace), n, ALGO[algo], _stream(stream)),
           "sort_pairs_device (status)")


def wave_tile_sort(d_keys, n: int, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_wave_tile_sort(_ptr(d_keys), n, KEY[key], _stream(stream)), "wave_tile_sort")


def tile_sort(d_in, d_out, n: int, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_tile_sort(_ptr(d_in), _ptr(d_out), n, KEY[key], _stream(stream)), "tile_sort")


def merge_pass(d_in, d_out, n: int, run: int, d_part, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_merge_pass(_ptr(d_in), _ptr(d_out), n, run, KEY[key], _ptr(d_part), _stream(stream)),
           "merge_pass")


def merge(d_a, la: int, d_b, lb: int, d_out, d0: int, d1: int, d_part, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_merge(_ptr(d_a) if la else 0, la, _ptr(d_b) if lb else 0, lb, _ptr(d_out), d0, d1,
                             KEY[key], _ptr(d_part), _stream(stream)), "merge")


def merge_runs_workspace_bytes(n: int) -> int:
    return int(lib.labsort_merge_runs_workspace_bytes(n))


def merge_runs(d_in, d_out, offsets, key: str = "u32", workspace=None, stream=None) -> None:
    """K-way merge (K <= 8) of the sorted runs d_in[offsets[q]:offsets[q+1]] into
    d_out[offsets[0]:offsets[-1]] (stable: equal keys keep run order)."""
    offs = [int(x) for x in offsets]
    if workspace is None:
        import torch
        workspace = torch.empty(max(merge_runs_workspace_bytes(offs[-1]), 1), dtype=torch.uint8, device="cuda")
    wsb = workspace.numel() * workspace.element_size()
    arr = (ctypes.c_size_t * len(offs))(*offs)
    _check(lib.labsort_merge_runs(_ptr(d_in), _ptr(d_out), arr, len(offs) - 1, KEY[key], _ptr(workspace), wsb,
                                  _stream(stream)), "merge_runs")


def pairs_workspace_bytes(n: int, algo: str = "radix") -> int:
    return int(lib.labsort_pairs_workspace_bytes(n, ALGO[algo]))


def pair_tile_keys() -> int:
    return int(lib.labsort_pair_tile_keys())


def sort_pairs_device(d_keys_in, d_vals_in, d_keys_out, d_vals_out, n: int, key: str = "u32", algo: str = "radix",
                      workspace=None, stream=None) -> None:
    """Stable sort of n (key, 4-byte payload) pairs (sort_by_key); equal keys keep
    their input order.  algo: "radix", "merge" or "auto".  Asynchronous on `stream`."""
    workspace, wsb, own = _workspace(workspace, lambda: pairs_workspace_bytes(n, algo))
    _check(lib.labsort_sort_pairs_device(_ptr(d_keys_in), _ptr(d_vals_in), _ptr(d_keys_out), _ptr(d_vals_out), n,
                                         KEY[key], ALGO[algo], _ptr(workspace), wsb, _stream(stream)),
           "sort_pairs_device")
    if own:
        pairs_workspace_status(workspace, n, algo, stream)


# ---- segmented sort: segment i = [offsets[i], offsets[i+1]) of one buffer ---------------
def segment_tile_keys() -> int:
    """Longest segment the one-pass LDS path sorts (keys only)."""
    return int(lib.labsort_segment_tile_keys())


def segment_pair_tile_keys() -> int:
    """Longest segment the one-pass LDS path sorts (key + payload)."""
    return int(lib.labsort_segment_pair_tile_keys())


def segment_class_edges(pairs: bool = False) -> list:
    """Upper length bound of each LDS class, ascending; the last is the tile size."""
    e = (ctypes.c_size_t * 8)()
    k = lib.labsort_segment_class_edges(1 if pairs else 0, e, 8)
    return [int(e[j]) for j in range(k)]


def segments_workspace_bytes(n: int, nseg: int, max_segment_keys: int = 0, pairs: bool = False) -> int:
    return int(lib.labsort_segments_workspace_bytes(n, nseg, max_segment_keys, 1 if pairs else 0))


def row_offsets(rows: int, cols: int, device="cuda"):
    """uint32 offsets (as an int32 tensor of rows + 1 words) of a row-major rows x cols matrix."""
    import torch
    assert rows * cols < 2**31
    return (torch.arange(rows + 1, dtype=torch.int64, device=device) * cols).to(torch.int32)


def sort_segments_device(d_in, d_out, n: int, d_offsets, nseg: int, max_segment_keys: int = 0, key: str = "u32",
                         workspace=None, stream=None) -> None:
    """Sort each segment [offsets[i], offsets[i+1]) of d_in into d_out (may alias) on `stream`.
    max_segment_keys: the longest segment (<= segment_tile_keys(): one LDS pass; 0 or longer:
    the general path).  With a caller-owned `workspace` the call stays asynchronous (check
    segments_workspace_status when the result is needed); without one it allocates, synchronises
    and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: segments_workspace_bytes(n, nseg, max_segment_keys))
    _check(lib.labsort_sort_segments_device(_ptr(d_in), _ptr(d_out), n, _ptr(d_offsets), nseg, max_segment_keys,
                                            KEY[key], _ptr(workspace), wsb, _stream(stream)), "sort_segments_device")
    if own:
        segments_workspace_status(workspace, stream)


def sort_segments_pairs_device(d_keys_in, d_vals_in, d_keys_out, d_vals_out, n: int, d_offsets, nseg: int,
                               max_segment_keys: int = 0, key: str = "u32", workspace=None, stream=None) -> None:
    """As sort_segments_device for (key, 4-byte payload) pairs; stable within each segment."""
    workspace, wsb, own = _workspace(workspace, lambda: segments_workspace_bytes(n, nseg, max_segment_keys, True))
    _check(lib.labsort_sort_segments_pairs_device(_ptr(d_keys_in), _ptr(d_vals_in), _ptr(d_keys_out), _ptr(d_vals_out),
                                                  n, _ptr(d_offsets), nseg, max_segment_keys, KEY[key], _ptr(workspace),
                                                  wsb, _stream(stream)), "sort_segments_pairs_device")
    if own:
        segments_workspace_status(workspace, stream)


def segments_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_ARG if the last segmented sort on
    `workspace` rejected its offsets, ERR_DEVICE if an inner sort reported a failure."""
    _check(lib.labsort_segments_workspace_status(_ptr(workspace), _stream(stream)), "sort_segments (status)")


def topk_workspace_bytes(rows: int, cols: int, k: int) -> int:
    return int(lib.labsort_topk_workspace_bytes(rows, cols, k))


def topk_device(d_keys, rows: int, cols: int, k: int, d_keys_out, d_idx_out=None, largest: bool = False,
                key: str = "u32", workspace=None, stream=None) -> None:
    """The k smallest (largest) keys of every row of the dense rows x cols matrix d_keys, best
    first, into d_keys_out (rows x k), and their positions within the row into d_idx_out (rows x k
    int32 / uint32 words, or None): torch.topk(x, k, largest=..., sorted=True) with the tie order
    fixed (equal keys in order of position; of the k-th key's ties the lowest positions).  key="f32":
    float32 tensors as they are, NaNs the largest keys and equal to each other, -0.0 below +0.0;
    key="bf16" / "f16": the same for torch.bfloat16 / torch.float16 tensors (d_keys and d_keys_out hold
    16-bit elements, d_idx_out stays 32-bit).  With a
    caller-owned `workspace` the call stays asynchronous (check topk_workspace_status when the
    result is needed); without one it allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: topk_workspace_bytes(rows, cols, k))
    _check(lib.labsort_topk_device(_ptr(d_keys), rows, cols, k, 1 if largest else 0, KEY[key], _ptr(d_keys_out),
                                   None if d_idx_out is None else _ptr(d_idx_out), _ptr(workspace), wsb,
                                   _stream(stream)), "topk_device")
    if own:
        topk_workspace_status(workspace, stream)


def _dense_rows(what: str, x, wide: bool = False):
    """(rows, cols, key) of the tensor topk(), kthvalue() and sort() take, or their TypeError.  wide:
    the caller also takes the 8-byte dtypes (sort and argsort alone)."""
    import torch
    keys = {torch.int32: "i32", torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
    if wide and hasattr(lib, "labsort_sort64_device"):  # (an older build loaded through LABSORT_LIBRARY has none)
        keys.update({torch.int64: "i64", torch.float64: "f64"})
        if hasattr(torch, "uint64"):
            keys[torch.uint64] = "u64"
    if not isinstance(x, torch.Tensor) or x.dtype not in keys:
        names = "int32, float32, bfloat16" + (", float16, int64, uint64 or float64" if wide else " or float16")
        raise TypeError(f"{what}: {names} tensor expected, got {getattr(x, 'dtype', type(x))}")
    if x.dim() not in (1, 2) or not x.is_contiguous():
        raise TypeError(f"{what}: a contiguous 1-D or 2-D tensor expected")
    if not x.is_cuda:
        raise TypeError(f"{what}: a CUDA tensor expected")
    rows, cols = (1, x.shape[0]) if x.dim() == 1 else x.shape
    return rows, cols, keys[x.dtype]


def topk(x, k: int, largest: bool = True, workspace=None, stream=None):
    """(values, indices) of the k largest (smallest) keys of every row of x, best first: topk_device
    with its outputs allocated.  x: a contiguous 1-D (one row) or 2-D CUDA tensor of dtype int32,
    float32, bfloat16 or float16; values has x's dtype and shape (rows, k), indices is int32 (rows, k).
    TypeError for another dtype or a non-contiguous tensor, before the device is touched.  Workspace
    and status as topk_device."""
    import torch
    rows, cols, key = _dense_rows("topk", x)
    values = torch.empty((rows, k), dtype=x.dtype, device=x.device)
    indices = torch.empty((rows, k), dtype=torch.int32, device=x.device)
    topk_device(x, rows, cols, k, values, indices, largest=largest, key=key, workspace=workspace, stream=stream)
    return values, indices


def topk_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_DEVICE if an inner sort of the last
    topk_device call on `workspace` reported a failure."""
    _check(lib.labsort_topk_workspace_status(_ptr(workspace), _stream(stream)), "topk (status)")


def sort_rows_workspace_bytes(rows: int, cols: int) -> int:
    return int(lib.labsort_sort_rows_workspace_bytes(rows, cols))


def sort_rows_device(d_keys, rows: int, cols: int, d_keys_out, d_idx_out=None, descending: bool = False,
                     key: str = "u32", workspace=None, stream=None) -> None:
    """Every row of the dense rows x cols matrix d_keys sorted into d_keys_out (rows x cols), stably,
    ascending or descending, and the keys' positions within their row into d_idx_out (rows x cols
    int32 / uint32 words, or None): torch.sort(x, dim=-1, descending=..., stable=True), topk_device's
    contract with k = cols.  key: "u32", "i32", "f32", "bf16" or "f16" (16-bit elements in d_keys and
    d_keys_out, d_idx_out stays 32-bit); NaNs are the largest keys and equal to each other, -0.0 is
    below +0.0.  Workspace and status as topk_device: with a caller-owned `workspace` the call stays
    asynchronous (check sort_rows_workspace_status when the result is needed); without one it
    allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: sort_rows_workspace_bytes(rows, cols))
    _check(lib.labsort_sort_rows_device(_ptr(d_keys), rows, cols, 1 if descending else 0, KEY[key], _ptr(d_keys_out),
                                        None if d_idx_out is None else _ptr(d_idx_out), _ptr(workspace), wsb,
                                        _stream(stream)), "sort_rows_device")
    if own:
        sort_rows_workspace_status(workspace, stream)


def sort_rows_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_DEVICE if an inner sort of the last
    sort_rows_device call on `workspace` reported a failure (rows past the LDS tile only)."""
    _check(lib.labsort_sort_rows_workspace_status(_ptr(workspace), _stream(stream)), "sort_rows (status)")


def sort16_chunk_keys() -> int:
    """Keys per (row, chunk) workgroup of sort16_device's long path."""
    return int(lib.labsort_sort16_chunk_keys())


def sort16_workspace_bytes(rows: int, cols: int, positions: bool = True) -> int:
    return int(lib.labsort_sort16_workspace_bytes(rows, cols, 1 if positions else 0))


def sort16_device(d_keys, rows: int, cols: int, d_keys_out, d_idx_out=None, descending: bool = False,
                  key: str = "bf16", workspace=None, stream=None) -> None:
    """sort_rows_device for key="bf16" / "f16" alone, with a path of its own for rows longer than
    segment_tile_keys(): two radix passes over the 16-bit keys and their positions on a workspace of
    about 6 bytes per key (2 without positions) instead of top-k's whole-row sort.  Keys and positions
    are bit-identical to sort_rows_device's.  Workspace and status as sort_rows_device: with a
    caller-owned `workspace` (>= sort16_workspace_bytes(rows, cols, d_idx_out is not None)) the call
    stays asynchronous; without one it allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: sort16_workspace_bytes(rows, cols, d_idx_out is not None))
    _check(lib.labsort_sort16_device(_ptr(d_keys), rows, cols, 1 if descending else 0, KEY[key], _ptr(d_keys_out),
                                     None if d_idx_out is None else _ptr(d_idx_out), _ptr(workspace), wsb,
                                     _stream(stream)), "sort16_device")
    if own:
        sort16_workspace_status(workspace, stream)


def sort16_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream` and check the workspace's status word, as sort_rows_workspace_status
    (no kernel of sort16_device sets it)."""
    _check(lib.labsort_sort16_workspace_status(_ptr(workspace), _stream(stream)), "sort16 (status)")


def sort64_chunk_keys() -> int:
    """C: keys per (row, chunk) workgroup of sort64_device; rows of up to C keys are sorted by one
    workgroup in LDS."""
    return int(lib.labsort_sort64_chunk_keys())


def sort64_workspace_bytes(rows: int, cols: int, positions: bool = True) -> int:
    return int(lib.labsort_sort64_workspace_bytes(rows, cols, 1 if positions else 0))


def sort64_device(d_keys, rows: int, cols: int, d_keys_out, d_idx_out=None, descending: bool = False,
                  key: str = "i64", workspace=None, stream=None) -> None:
    """sort_rows_device's contract for key="u64" / "i64" / "f64" alone: d_keys and d_keys_out hold 8-byte
    elements, d_idx_out stays 32-bit.  Stable radix passes with 8-bit digits over the keys' 64-bit
    order images, of which only those whose digit varies run (decided on the device: keys below 2^32
    take four passes).  Workspace and status as sort_rows_device: with a caller-owned `workspace` (>=
    sort64_workspace_bytes(rows, cols, d_idx_out is not None)) the call stays asynchronous; without
    one it allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: sort64_workspace_bytes(rows, cols, d_idx_out is not None))
    _check(lib.labsort_sort64_device(_ptr(d_keys), rows, cols, 1 if descending else 0, KEY[key], _ptr(d_keys_out),
                                     None if d_idx_out is None else _ptr(d_idx_out), _ptr(workspace), wsb,
                                     _stream(stream)), "sort64_device")
    if own:
        sort64_workspace_status(workspace, stream)


def sort64_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream` and check the workspace's status word, as sort_rows_workspace_status
    (no kernel of sort64_device sets it)."""
    _check(lib.labsort_sort64_workspace_status(_ptr(workspace), _stream(stream)), "sort64 (status)")


def sort64_passes(workspace, stream=None) -> int:
    """Synchronise `stream`; the plan of the last sort64_device call on `workspace` as a bitmask: bit p
    set if the pass on byte p of the order image ran.  0 after a call with cols <= sort64_chunk_keys()
    (each row plans for itself in LDS)."""
    r = int(lib.labsort_sort64_passes(_ptr(workspace), _stream(stream)))
    if r < 0:
        _check(-r, "sort64_passes")
    return r


def _sort16_routed(rows: int, cols: int, key: str, workspace) -> bool:
    """Does sort() hand this call to sort16_device?  bfloat16 / float16 rows past the LDS tile, when
    the caller passed no workspace (one sized by sort_rows_workspace_bytes belongs to
    sort_rows_device's route, which stays for it)."""
    return (key in ("bf16", "f16") and workspace is None and cols > segment_tile_keys()
            and hasattr(lib, "labsort_sort16_device"))  # (an older build loaded through LABSORT_LIBRARY has none)


def sort(x, descending: bool = False, workspace=None, stream=None):
    """(values, indices) of every row of x sorted, stably: sort_rows_device with its outputs allocated.
    x: a contiguous 1-D (one row) or 2-D CUDA tensor of dtype int32, float32, bfloat16 or float16;
    values has x's dtype and shape, indices is int32 of the same shape.  TypeError for another dtype,
    a non-contiguous or a CPU tensor, before the device is touched.  Workspace and status as
    sort_rows_device.  bfloat16 / float16 rows longer than segment_tile_keys() without a caller's
    workspace are sorted by sort16_device: the same result by contract.  int64, float64 and (where
    torch has it) uint64 tensors are sorted by sort64_device; a caller's workspace for them is one
    sized by sort64_workspace_bytes.  indices is int32 for every dtype."""
    import torch
    rows, cols, key = _dense_rows("sort", x, wide=True)
    values = torch.empty_like(x)
    indices = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    if key in ("u64", "i64", "f64"):
        sort64_device(x, rows, cols, values, indices, descending=descending, key=key, workspace=workspace, stream=stream)
    elif _sort16_routed(rows, cols, key, workspace):
        sort16_device(x, rows, cols, values, indices, descending=descending, key=key, stream=stream)
    else:
        sort_rows_device(x, rows, cols, values, indices, descending=descending, key=key, workspace=workspace,
                         stream=stream)
    return values, indices


def argsort(x, descending: bool = False, workspace=None, stream=None):
    """The indices of sort(x, descending): the stable argsort of every row."""
    return sort(x, descending=descending, workspace=workspace, stream=stream)[1]


def kth_row_keys() -> int:
    """Longest row kth_device selects in one launch (the row held in one workgroup's registers)."""
    return int(lib.labsort_kth_row_keys())


def kth_workspace_bytes(rows: int, cols: int) -> int:
    return int(lib.labsort_kth_workspace_bytes(rows, cols))


def _is_k_tensor(k) -> bool:
    return hasattr(k, "data_ptr")


def kth_device(d_keys, rows: int, cols: int, k, d_keys_out, d_idx_out=None, largest: bool = False, key: str = "u32",
               workspace=None, stream=None) -> None:
    """The k-th smallest (largest) key of every row of the dense rows x cols matrix d_keys into
    d_keys_out (rows elements), and its position within the row into d_idx_out (rows int32 / uint32
    words, or None): column k - 1 of sort_rows_device(descending=largest), bit for bit, without the
    sort.  k is an int (1 <= k <= cols, every row), or an int32 CUDA tensor of `rows` elements, one k per
    row, which is passed as d_k: a value outside [1, cols] is clamped on the device and reported by
    kth_workspace_status as ERR_ARG, the other rows' results stay valid.  key as topk_device.  Workspace
    and status follow topk_device: with a caller-owned `workspace` (>= kth_workspace_bytes(rows, cols))
    the call stays asynchronous; without one it allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: kth_workspace_bytes(rows, cols))
    d_k = _ptr(k) if _is_k_tensor(k) else None
    _check(lib.labsort_kth_device(_ptr(d_keys), rows, cols, 0 if d_k is not None else int(k), d_k, 1 if largest else 0,
                                  KEY[key], _ptr(d_keys_out), None if d_idx_out is None else _ptr(d_idx_out),
                                  _ptr(workspace), wsb, _stream(stream)), "kth_device")
    if own:
        kth_workspace_status(workspace, stream)


def kth_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_ARG if a row's k of the last kth_device call on
    `workspace` lay outside [1, cols] (that row's result is the clamped k's)."""
    _check(lib.labsort_kth_workspace_status(_ptr(workspace), _stream(stream)), "kth (status)")


def kthvalue(x, k, largest: bool = False, workspace=None, stream=None):
    """(values, indices) of the k-th smallest (largest) key of every row of x: kth_device with its
    outputs allocated (torch.kthvalue(x, k, dim=-1) with the tie order fixed: of the k-th key's ties the
    one that a stable sort puts k-th).  x: a contiguous 1-D (one row) or 2-D CUDA tensor of dtype int32,
    float32, bfloat16 or float16; k: an int, or a contiguous int32 CUDA tensor of `rows` elements (one k
    per row).  values has x's dtype and shape (rows,), indices is int32 (rows,).  TypeError before the
    device is touched for another dtype, a non-contiguous or CPU tensor, or a k tensor that is not a
    contiguous int32 CUDA tensor of `rows` elements.  The lower median of a row is k = (cols + 1) // 2.
    NaNs are the largest keys here and equal to each other, so a row with NaNs still has a finite median
    when fewer than half of its keys are NaN, where torch.median returns NaN.  Workspace and status as
    kth_device."""
    import torch
    rows, cols, key = _dense_rows("kthvalue", x)
    if isinstance(k, torch.Tensor):
        if k.dtype != torch.int32 or not k.is_cuda or not k.is_contiguous() or k.dim() != 1 or k.shape[0] != rows:
            raise TypeError(f"kthvalue: k must be an int or a contiguous int32 CUDA tensor of {rows} elements")
    elif isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"kthvalue: k must be an int or an int32 CUDA tensor, got {type(k)}")
    values = torch.empty((rows,), dtype=x.dtype, device=x.device)
    indices = torch.empty((rows,), dtype=torch.int32, device=x.device)
    kth_device(x, rows, cols, k, values, indices, largest=largest, key=key, workspace=workspace, stream=stream)
    return values, indices


def topk_mask_workspace_bytes(rows: int, cols: int) -> int:
    return int(lib.labsort_topk_mask_workspace_bytes(rows, cols))


def topk_mask_device(d_keys, rows: int, cols: int, k, d_keys_out=None, d_mask_out=None, largest: bool = False,
                     fill_bits: int = 0, key: str = "u32", workspace=None, stream=None) -> None:
    """Top-k filtering of every row of the dense rows x cols matrix d_keys: element i of row r is kept
    iff it is among the row's k smallest (largest) keys, equal keys in order of position, so that
    exactly k elements of the row are kept (the first k columns of sort_rows_device(descending=largest)'s
    positions, as a set).  d_keys_out (rows x cols elements, or None): the kept keys where they were,
    `fill_bits` (a word of the key type) everywhere else; d_keys_out may be d_keys itself (in place).
    d_mask_out (rows x cols bytes, torch.bool's layout, or None): 1 where kept.  At least one of the two.
    k as for kth_device: an int, or an int32 CUDA tensor of `rows` elements (a value outside [1, cols] is
    clamped and reported by topk_mask_workspace_status).  key as topk_device.  Workspace and status follow
    kth_device: with a caller-owned `workspace` (>= topk_mask_workspace_bytes(rows, cols)) the call stays
    asynchronous; without one it allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: topk_mask_workspace_bytes(rows, cols))
    d_k = _ptr(k) if _is_k_tensor(k) else None
    _check(lib.labsort_topk_mask_device(_ptr(d_keys), rows, cols, 0 if d_k is not None else int(k), d_k,
                                        1 if largest else 0, KEY[key], int(fill_bits) & 0xFFFFFFFF,
                                        None if d_keys_out is None else _ptr(d_keys_out),
                                        None if d_mask_out is None else _ptr(d_mask_out),
                                        _ptr(workspace), wsb, _stream(stream)), "topk_mask_device")
    if own:
        topk_mask_workspace_status(workspace, stream)


def topk_mask_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_ARG if a row's k of the last topk_mask_device
    call on `workspace` lay outside [1, cols] (that row is filtered with the clamped k)."""
    _check(lib.labsort_topk_mask_workspace_status(_ptr(workspace), _stream(stream)), "topk_mask (status)")


def _topk_filter_args(what: str, x, k):
    """(rows, cols, key) for topk_filter() and topk_mask(), or kthvalue()'s TypeErrors."""
    import torch
    rows, cols, key = _dense_rows(what, x)
    if isinstance(k, torch.Tensor):
        if k.dtype != torch.int32 or not k.is_cuda or not k.is_contiguous() or k.dim() != 1 or k.shape[0] != rows:
            raise TypeError(f"{what}: k must be an int or a contiguous int32 CUDA tensor of {rows} elements")
    elif isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{what}: k must be an int or an int32 CUDA tensor, got {type(k)}")
    return rows, cols, key


def _fill_bits(dtype, fill) -> int:
    """The word of one element of `dtype` that holds `fill`."""
    import torch
    t = torch.tensor([fill], dtype=dtype)
    if dtype in (torch.bfloat16, torch.float16):
        return int(t.view(torch.int16).item()) & 0xFFFF
    return int(t.view(torch.int32).item()) & 0xFFFFFFFF


def topk_filter(x, k, largest: bool = True, fill=None, out=None, workspace=None, stream=None):
    """x with everything outside each row's top k replaced by `fill`: topk_mask_device with the keys
    output (what a sampler does to its logits before the softmax).  x: what kthvalue takes; k: an int, or
    a contiguous int32 CUDA tensor of `rows` elements (one k per row).  Exactly k elements of every row
    are kept, equal keys in order of position; a kept NaN comes back as the canonical NaN.  fill: by
    default the worst value for the direction (-inf for largest, +inf otherwise; int32: the dtype's
    min / max).  out: None (allocated), x itself (in place) or another contiguous tensor of x's shape
    and dtype; it is returned.  TypeError before the device is touched for what kthvalue rejects and for
    a wrong `out`.  Workspace and status as topk_mask_device."""
    import torch
    rows, cols, key = _topk_filter_args("topk_filter", x, k)
    if out is None:
        out = torch.empty_like(x)
    elif (not isinstance(out, torch.Tensor) or out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous()
          or out.device != x.device):
        raise TypeError("topk_filter: out must be None, x itself or a contiguous tensor of x's shape, dtype and device")
    if fill is None:
        if x.dtype == torch.int32:
            fill = torch.iinfo(torch.int32).min if largest else torch.iinfo(torch.int32).max
        else:
            fill = float("-inf") if largest else float("inf")
    topk_mask_device(x, rows, cols, k, d_keys_out=out, largest=largest, fill_bits=_fill_bits(x.dtype, fill), key=key,
                     workspace=workspace, stream=stream)
    return out


def topk_mask(x, k, largest: bool = True, workspace=None, stream=None):
    """The torch.bool tensor of x's shape that is True at each row's top k elements (topk_filter's
    rule: exactly k per row, equal keys in order of position).  Arguments as topk_filter."""
    import torch
    rows, cols, key = _topk_filter_args("topk_mask", x, k)
    mask = torch.empty(x.shape, dtype=torch.bool, device=x.device)
    topk_mask_device(x, rows, cols, k, d_mask_out=mask, largest=largest, key=key, workspace=workspace, stream=stream)
    return mask


def top_p_weight(word: int, key: str = "f32") -> int:
    """The fixed-point weight of one key word in top_p_device: min(floor(x 2^40), 2^40), 0 for a set sign
    bit and for a NaN (labsort_top_p_weight; 0 for a key type other than f32, bf16, f16)."""
    return int(lib.labsort_top_p_weight(int(word) & 0xFFFFFFFF, KEY[key]))


def top_p_workspace_bytes(rows: int, cols: int) -> int:
    return int(lib.labsort_top_p_workspace_bytes(rows, cols))


def top_p_device(d_keys, rows: int, cols: int, p, d_keys_out=None, d_mask_out=None, d_kept_out=None,
                 fill_bits: int = 0, key: str = "f32", workspace=None, stream=None) -> None:
    """Top-p filtering of every row of the dense rows x cols matrix d_keys of non-negative weights
    (probabilities): the row keeps the smallest prefix of sort_rows_device(descending=True)'s order
    whose weights, summed exactly in 2^-40 fixed point, reach p times the row's total (labsort.h has the
    rule).  d_keys_out (rows x cols elements, or None; may be d_keys itself): the kept keys where they
    were, `fill_bits` elsewhere.  d_mask_out (rows x cols bytes, or None): 1 where kept.  d_kept_out (rows
    uint32 words, or None): how many elements each row keeps.  At least one of the three.  p is a float in
    (0, 1], or a float32 CUDA tensor of `rows` elements, one p per row, which is passed as d_p: a value
    outside (0, 1] is clamped on the device and reported by top_p_workspace_status as ERR_ARG, as is a row
    whose weights are all zero (it is kept whole); the other rows stay valid.  key: f32, bf16 or f16.
    Workspace and status follow topk_mask_device: with a caller-owned `workspace`
    (>= top_p_workspace_bytes(rows, cols)) the call stays asynchronous; without one it allocates,
    synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: top_p_workspace_bytes(rows, cols))
    d_p = _ptr(p) if _is_k_tensor(p) else None
    _check(lib.labsort_top_p_device(_ptr(d_keys), rows, cols, 1.0 if d_p is not None else float(p), d_p, KEY[key],
                                    int(fill_bits) & 0xFFFFFFFF,
                                    None if d_keys_out is None else _ptr(d_keys_out),
                                    None if d_mask_out is None else _ptr(d_mask_out),
                                    None if d_kept_out is None else _ptr(d_kept_out),
                                    _ptr(workspace), wsb, _stream(stream)), "top_p_device")
    if own:
        top_p_workspace_status(workspace, stream)


def top_p_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_ARG if in the last top_p_device call on
    `workspace` a row's p lay outside (0, 1] (it was clamped) or a row's weights were all zero (the
    row was kept whole)."""
    _check(lib.labsort_top_p_workspace_status(_ptr(workspace), _stream(stream)), "top_p (status)")


def _top_p_args(what: str, x, p):
    """(rows, cols, key) for top_p_filter() and top_p_mask(), or their TypeErrors."""
    import torch
    if isinstance(x, torch.Tensor) and x.dtype == torch.int32:
        raise TypeError(f"{what}: float32, bfloat16 or float16 tensor expected, got {x.dtype}")
    rows, cols, key = _dense_rows(what, x)
    if isinstance(p, torch.Tensor):
        if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.dim() != 1 or p.shape[0] != rows:
            raise TypeError(f"{what}: p must be a float or a contiguous float32 CUDA tensor of {rows} elements")
    elif isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: p must be a float or a float32 CUDA tensor, got {type(p)}")
    return rows, cols, key


def top_p_filter(x, p, fill=0.0, out=None, return_kept: bool = False, workspace=None, stream=None):
    """x with everything outside each row's top-p set replaced by `fill`: top_p_device with the keys
    output (what a sampler does to its probabilities after the softmax).  x: a contiguous 1-D (one row)
    or 2-D CUDA tensor of float32, bfloat16 or float16; p: a float in (0, 1], or a contiguous float32 CUDA
    tensor of `rows` elements (one p per row).  out: None (allocated), x itself (in place) or another
    contiguous tensor of x's shape and dtype; it is returned.  return_kept: also return the int32 tensor
    of `rows` elements that holds how many elements each row keeps.  TypeError before the device is
    touched for anything else.  The sums are exact integers, so the result does not depend on their
    order and repeats bit for bit.  Workspace and status as top_p_device."""
    import torch
    rows, cols, key = _top_p_args("top_p_filter", x, p)
    if out is None:
        out = torch.empty_like(x)
    elif (not isinstance(out, torch.Tensor) or out.dtype != x.dtype or out.shape != x.shape or not out.is_contiguous()
          or out.device != x.device):
        raise TypeError("top_p_filter: out must be None, x itself or a contiguous tensor of x's shape, dtype and device")
    kept = torch.empty((rows,), dtype=torch.int32, device=x.device) if return_kept else None
    top_p_device(x, rows, cols, p, d_keys_out=out, d_kept_out=kept, fill_bits=_fill_bits(x.dtype, fill), key=key,
                 workspace=workspace, stream=stream)
    return (out, kept) if return_kept else out


def top_p_mask(x, p, return_kept: bool = False, workspace=None, stream=None):
    """The torch.bool tensor of x's shape that is True at each row's top-p set (top_p_filter's rule),
    with return_kept also the int32 count per row.  Arguments as top_p_filter."""
    import torch
    rows, cols, key = _top_p_args("top_p_mask", x, p)
    mask = torch.empty(x.shape, dtype=torch.bool, device=x.device)
    kept = torch.empty((rows,), dtype=torch.int32, device=x.device) if return_kept else None
    top_p_device(x, rows, cols, p, d_mask_out=mask, d_kept_out=kept, key=key, workspace=workspace, stream=stream)
    return (mask, kept) if return_kept else mask


def sample_workspace_bytes(rows: int, cols: int, ndraw: int) -> int:
    return int(lib.labsort_sample_workspace_bytes(rows, cols, ndraw))


def sample_device(d_keys, rows: int, cols: int, d_u, ndraw: int, d_idx_out, key: str = "f32", workspace=None,
                  stream=None) -> None:
    """Categorical sampling from every row of the dense rows x cols matrix d_keys of non-negative weights
    (probabilities, normalised or not; never written): d_idx_out[r, d] (rows x ndraw uint32 words) is the
    position drawn for the random word d_u[r, d] (rows x ndraw uint32 words, uniform in [0, 2^32), supplied
    by the caller, never written) by exact inverse CDF: with top_p_device's integer weights w and the row's
    total W, the smallest j whose inclusive prefix w_0 + .. + w_j exceeds floor(U W / 2^32) (labsort.h has
    the rule).  An element of weight zero (a NaN, a negative, anything below 2^-40) is never drawn.  A row
    without mass draws 0xFFFFFFFF and is reported by sample_workspace_status as ERR_ARG; the other rows
    stay valid.  key: f32, bf16 or f16.  Workspace and status follow top_p_device: with a caller-owned
    `workspace` (>= sample_workspace_bytes(rows, cols, ndraw)) the call stays asynchronous; without one it
    allocates, synchronises and checks."""
    workspace, wsb, own = _workspace(workspace, lambda: sample_workspace_bytes(rows, cols, ndraw))
    _check(lib.labsort_sample_device(_ptr(d_keys), rows, cols, _ptr(d_u), ndraw, KEY[key], _ptr(d_idx_out),
                                     _ptr(workspace), wsb, _stream(stream)), "sample_device")
    if own:
        sample_workspace_status(workspace, stream)


def sample_workspace_status(workspace, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_ARG if in the last sample_device call on
    `workspace` a row's weights were all zero (its draws are 0xFFFFFFFF)."""
    _check(lib.labsort_sample_workspace_status(_ptr(workspace), _stream(stream)), "sample (status)")


def sample(x, num_samples: int = 1, u=None, generator=None, workspace=None, stream=None):
    """The int32 tensor of shape (rows, num_samples) of positions drawn from every row of x by its
    weights, with replacement: sample_device with its output allocated (what torch.multinomial(x,
    num_samples, replacement=True) does, as exact integer arithmetic).  x: a contiguous 1-D (one row)
    or 2-D CUDA tensor of float32, bfloat16 or float16.  u: None, or a contiguous tensor of shape
    (rows, num_samples) on x's device: int32 or uint32 are the random words themselves, float32 values in
    [0, 1) are taken as floor(u 2^32) (exact in float64); a value below 0 and a NaN are taken as word 0, a
    value of 1 or more as word 2^32 - 1.  u=None draws the words with torch on x's
    device from `generator`: two 16-bit halves from torch.randint, since one call does not reach 2^32.
    TypeError before the device is touched for anything else.  Equal words give equal draws, bit for
    bit.  Workspace and status as sample_device."""
    import torch
    if isinstance(x, torch.Tensor) and x.dtype == torch.int32:
        raise TypeError(f"sample: float32, bfloat16 or float16 tensor expected, got {x.dtype}")
    rows, cols, key = _dense_rows("sample", x)
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 0:
        raise TypeError(f"sample: num_samples must be a non-negative int, got {num_samples!r}")
    ndraw = int(num_samples)
    if cols == 0:
        raise TypeError("sample: x has no columns to draw from")
    if u is None:
        hi = torch.randint(0, 1 << 16, (rows, ndraw), dtype=torch.int32, device=x.device, generator=generator)
        lo = torch.randint(0, 1 << 16, (rows, ndraw), dtype=torch.int32, device=x.device, generator=generator)
        words = (hi << 16) | lo  # (int32 wraps: the bits are the word)
    else:
        word_dtypes = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])
        if (not isinstance(u, torch.Tensor) or u.dtype not in word_dtypes + [torch.float32] or u.device != x.device
                or not u.is_contiguous() or tuple(u.shape) != (rows, ndraw)):
            raise TypeError(f"sample: u must be None or a contiguous int32, uint32 or float32 tensor of shape ({rows}, {ndraw}) "
                            "on x's device")
        if u.dtype == torch.float32:
            words = (u.to(torch.float64) * 4294967296.0).floor().nan_to_num_(nan=0.0).clamp_(0.0, 4294967295.0).to(torch.int64).to(torch.int32)
        else:
            words = u
    out = torch.empty((rows, ndraw), dtype=torch.int32, device=x.device)
    if rows == 0 or ndraw == 0:
        return out  # (nothing is launched: there is no status to read)
    sample_device(x, rows, cols, words, ndraw, out, key=key, workspace=workspace, stream=stream)
    return out


def unique_chunk_keys() -> int:
    """C: elements per workgroup of unique_device's run-edge passes (the sorted array, or the input
    in consecutive mode, is cut into chunks of C)."""
    return int(lib.labsort_unique_chunk_keys())


def unique_workspace_bytes(n: int, key: str = "u32", consecutive: bool = False, positions: bool = True) -> int:
    """Workspace of unique_device for n keys; positions: d_first_out or d_inverse_out will be passed
    (a workspace sized with them serves a call without)."""
    return int(lib.labsort_unique_workspace_bytes(n, KEY[key], UNIQUE_CONSECUTIVE if consecutive else 0,
                                                  1 if positions else 0))


def unique_device(d_keys, n: int, d_unique_out, d_num_out, d_counts_out=None, d_first_out=None, d_inverse_out=None,
                  key: str = "u32", consecutive: bool = False, workspace=None, stream=None) -> None:
    """The distinct keys of d_keys[0..n) into d_unique_out (room for n elements of the key type; the
    first m are written, in ascending order), m into the one word d_num_out, and on request each
    key's number of occurrences (d_counts_out), the position of its first occurrence (d_first_out)
    and every element's index into d_unique_out (d_inverse_out): int32 / uint32 buffers of n words.
    key: "u32", "i32", "f32", "u64", "i64" or "f64"; keys are equal when their order images are, so
    every NaN is one value (written as 0x7FFF..) and -0.0 and +0.0 are two.  consecutive: nothing is
    sorted, entry j describes the j-th run of equal neighbours in input order.  d_keys is never
    written, nor anything past m in the outputs.  The call does not synchronise and reads nothing
    back, so it can be captured in a graph; without `workspace` one of unique_workspace_bytes(...)
    bytes is taken from torch's allocator, which orders its reuse on the current stream only.
    unique_workspace_status reports the inner sort's status once the result is needed."""
    pos = d_first_out is not None or d_inverse_out is not None
    workspace, wsb, _ = _workspace(workspace, lambda: unique_workspace_bytes(n, key, consecutive, pos))
    opt = lambda t: None if t is None else _ptr(t)  # noqa: E731
    _check(lib.labsort_unique_device(None if d_keys is None else _ptr(d_keys), n, KEY[key],
                                     UNIQUE_CONSECUTIVE if consecutive else 0, _ptr(d_unique_out), opt(d_counts_out),
                                     opt(d_first_out), opt(d_inverse_out), _ptr(d_num_out), _ptr(workspace), wsb,
                                     _stream(stream)), "unique_device")


def unique_workspace_status(workspace, n: int, key: str = "u32", consecutive: bool = False, stream=None) -> None:
    """Synchronise `stream`; raise LabsortError with ERR_DEVICE if the inner sort of the last
    unique_device(n, key, consecutive) call on `workspace` reported an error."""
    _check(lib.labsort_unique_workspace_status(_ptr(workspace), n, KEY[key], UNIQUE_CONSECUTIVE if consecutive else 0,
                                               _stream(stream)), "unique (status)")


def unique(x, return_inverse: bool = False, return_counts: bool = False, return_index: bool = False,
           consecutive: bool = False, workspace=None, stream=None):
    """The distinct values of x in ascending order (consecutive: the runs of equal neighbours in input
    order): unique_device with its outputs allocated.  x: a contiguous 1-D CUDA tensor of dtype int32,
    float32, int64 or float64, or torch.uint32 / torch.uint64 where torch has them.  Returns values,
    or the tuple (values, inverse, counts, index) of what was asked for, in that order (torch.unique's,
    with index last); inverse has x's length, the others m elements; all three are int32.  Equality
    is that of unique_device: on integers torch.unique's, on floats every NaN one value (torch keeps
    each) and -0.0 apart from +0.0 (torch merges them).  The number of distinct values is read back
    from the device to slice the outputs: one synchronisation of `stream`; unique_device has none.
    TypeError for another dtype, a tensor that is not 1-D and contiguous, or a CPU tensor, before the
    device is touched."""
    import torch
    keys = {torch.int32: "i32", torch.float32: "f32", torch.int64: "i64", torch.float64: "f64"}
    for name, key in (("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            keys[getattr(torch, name)] = key
    if not isinstance(x, torch.Tensor) or x.dtype not in keys:
        raise TypeError("unique: int32, float32, int64, float64, uint32 or uint64 tensor expected, "
                        f"got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 1 or not x.is_contiguous():
        raise TypeError("unique: a contiguous 1-D tensor expected")
    if not x.is_cuda:
        raise TypeError("unique: a CUDA tensor expected")
    n, key = x.shape[0], keys[x.dtype]
    words = lambda on: torch.empty(n, dtype=torch.int32, device=x.device) if on else None  # noqa: E731
    values = torch.empty_like(x)
    num = torch.empty(1, dtype=torch.int32, device=x.device)
    inverse, counts, index = words(return_inverse), words(return_counts), words(return_index)
    m = 0
    if n:  # (an empty tensor has no address to pass)
        pos = return_inverse or return_index
        workspace, _, _ = _workspace(workspace, lambda: unique_workspace_bytes(n, key, consecutive, pos))
        unique_device(x, n, values, num, counts, index, inverse, key=key, consecutive=consecutive, workspace=workspace,
                      stream=stream)
        unique_workspace_status(workspace, n, key, consecutive, stream)  # (synchronises)
        m = int(num.item())
    out = [values[:m]]
    if return_inverse:
        out.append(inverse)
    if return_counts:
        out.append(counts[:m])
    if return_index:
        out.append(index[:m])
    return out[0] if len(out) == 1 else tuple(out)


def searchsorted_row_keys(key: str = "u32") -> int:
    """The longest sequence that searchsorted_device stages in LDS (one launch, no workspace): 64 KB of
    images of the key type."""
    return int(lib.labsort_searchsorted_row_keys(KEY[key]))


def searchsorted_chunk_values() -> int:
    """V: values per workgroup step of searchsorted_device's kernels."""
    return int(lib.labsort_searchsorted_chunk_values())


def searchsorted_workspace_bytes(seq_rows: int, cols: int, key: str = "u32") -> int:
    """Workspace of searchsorted_device: 0 up to searchsorted_row_keys(key) columns, above that a header
    and one table of 4096 sample images per sequence."""
    return int(lib.labsort_searchsorted_workspace_bytes(seq_rows, cols, KEY[key]))


def searchsorted_device(d_sorted, seq_rows: int, cols: int, d_values, rows: int, nv: int, d_out, right: bool = False,
                        key: str = "u32", d_sorter=None, workspace=None, stream=None) -> None:
    """d_out[r][j] = the number of elements of the row's sequence whose order image is below (right:
    not above) that of d_values[r][j].  d_sorted: seq_rows x cols keys, every row ascending in image
    order, seq_rows == rows (row r searched in sequence r) or 1 (every value in the one sequence);
    d_values: rows x nv keys of the same type; d_out: rows x nv int32 / uint32 words; d_sorter: None or
    seq_rows x cols int32 positions that put the rows in order (argsort's output).  key: any of KEY.
    NaNs are one value past every number and -0.0 < +0.0.  The call does not synchronise and reads
    nothing back, so it can be captured in a graph; a workspace is needed past searchsorted_row_keys(key)
    columns only and is then, without `workspace`, taken from torch's allocator, which orders its
    reuse on the current stream only."""
    need = searchsorted_workspace_bytes(seq_rows, cols, key)
    wsb = 0
    if need or workspace is not None:
        workspace, wsb, _ = _workspace(workspace, lambda: need)
    opt = lambda t: None if t is None else _ptr(t)  # noqa: E731
    _check(lib.labsort_searchsorted_device(opt(d_sorted), seq_rows, cols, opt(d_sorter), opt(d_values), rows, nv,
                                           1 if right else 0, KEY[key], opt(d_out), opt(workspace), wsb,
                                           _stream(stream)), "searchsorted_device")


def _search_tensor(what: str, name: str, x):
    """The key of a tensor searchsorted() and bucketize() take, or the TypeError for its dtype."""
    import torch
    keys = {torch.int32: "i32", torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.int64: "i64",
            torch.float64: "f64"}
    for tname, key in (("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, tname):
            keys[getattr(torch, tname)] = key
    if not isinstance(x, torch.Tensor) or x.dtype not in keys:
        raise TypeError(f"{what}: {name}: int32, float32, bfloat16, float16, int64, float64, uint32 or uint64 tensor "
                        f"expected, got {getattr(x, 'dtype', type(x))}")
    return keys[x.dtype]


def searchsorted(sorted_sequence, values, right: bool = False, side=None, sorter=None, workspace=None, stream=None,
                 _what: str = "searchsorted"):
    """torch.searchsorted(sorted_sequence, values, out_int32=True) under the library's order:
    searchsorted_device with its output allocated.  Both are contiguous CUDA tensors of one dtype out
    of int32, float32, bfloat16, float16, int64, float64 and torch.uint32 / torch.uint64; the result is
    an int32 tensor of values' shape.  A 1-D sequence takes values of any shape; an N-D sequence needs
    values of N dimensions with the same leading ones, row by row.  sorter: a contiguous int32 CUDA
    tensor of the sequence's shape that puts it in order (argsort's).  side="right" means right=True;
    side="left" with right=True is a ValueError, as is an unknown side.  On integers and on floats free
    of NaNs and of zeros of both signs the result is torch's; a NaN is one value past every number and
    -0.0 < +0.0.  TypeError for a dtype that is not taken or differs between the two, a CPU tensor or a
    non-contiguous one; ValueError for shapes that do not match; all before the device is touched."""
    import torch
    if side is not None:
        if side not in ("left", "right"):
            raise ValueError(f"{_what}: side is 'left' or 'right', got {side!r}")
        if side == "left" and right:
            raise ValueError(f"{_what}: side='left' contradicts right=True")
        right = side == "right"
    key = _search_tensor(_what, "sorted_sequence", sorted_sequence)
    if _search_tensor(_what, "values", values) != key:
        raise TypeError(f"{_what}: sorted_sequence is {sorted_sequence.dtype}, values {values.dtype}: one dtype expected")
    seq = sorted_sequence
    if sorter is not None and (not isinstance(sorter, torch.Tensor) or sorter.dtype != torch.int32):
        raise TypeError(f"{_what}: sorter: int32 tensor expected, got {getattr(sorter, 'dtype', type(sorter))}")
    named = [("sorted_sequence", seq), ("values", values)] + ([("sorter", sorter)] if sorter is not None else [])
    for name, t in named:
        if not t.is_contiguous():
            raise TypeError(f"{_what}: {name}: a contiguous tensor expected")
    for name, t in named:
        if not t.is_cuda:
            raise TypeError(f"{_what}: {name}: a CUDA tensor expected")
    if seq.dim() < 1:
        raise ValueError(f"{_what}: a sequence of at least one dimension expected")
    if sorter is not None and sorter.shape != seq.shape:
        raise ValueError(f"{_what}: sorter has shape {tuple(sorter.shape)}, the sequence {tuple(seq.shape)}")
    cols = seq.shape[-1]
    if seq.dim() == 1:
        seq_rows, rows, nv = 1, 1, values.numel()
    else:
        if values.dim() != seq.dim() or values.shape[:-1] != seq.shape[:-1]:
            raise ValueError(f"{_what}: values of shape {tuple(values.shape)} do not match the leading dimensions of "
                             f"the sequence's {tuple(seq.shape)}")
        nv = values.shape[-1]
        rows = seq_rows = values.numel() // nv if nv else 0
    out = torch.empty(values.shape, dtype=torch.int32, device=values.device)
    if rows and nv:  # (an empty tensor has no address to pass)
        searchsorted_device(seq if cols else None, seq_rows, cols, values, rows, nv, out, right=right, key=key,
                            d_sorter=sorter if cols else None, workspace=workspace, stream=stream)
    return out


def bucketize(input, boundaries, right: bool = False, workspace=None, stream=None):  # noqa: A002
    """torch.bucketize(input, boundaries, out_int32=True, right=right): searchsorted(boundaries, input)
    for a 1-D tensor of boundaries, under the same order and with the same errors."""
    if getattr(boundaries, "dim", lambda: 1)() != 1:
        raise ValueError("bucketize: 1-D boundaries expected")
    return searchsorted(boundaries, input, right=right, workspace=workspace, stream=stream, _what="bucketize")


def bucket_counts_row_edges(key: str = "u32") -> int:
    """The longest edge row whose images bucket_counts_device keeps in LDS beside its counters (no
    workspace): 10176 4-byte, 6784 8-byte, 13632 2-byte edges."""
    return int(lib.labsort_bucket_counts_row_edges(KEY[key]))


def bucket_counts_workspace_bytes(edge_rows: int, nedges: int, key: str = "u32") -> int:
    """Workspace of bucket_counts_device: 0 up to bucket_counts_row_edges(key) edges, above that a header
    and one table of 4096 sample images per edge row."""
    return int(lib.labsort_bucket_counts_workspace_bytes(edge_rows, nedges, KEY[key]))


def bucket_counts_device(d_edges, edge_rows: int, nedges: int, d_values, rows: int, nv: int, d_counts_out, right: bool = False,
                         key: str = "u32", workspace=None, stream=None) -> None:
    """d_counts_out[r][b] = the number of values of row r that searchsorted_device with the same
    `right` ranks b in the row's edges: bin 0 lies below the first edge, bin nedges past the last, a
    value equal to an edge goes below it (right: above).  d_edges: edge_rows x nedges keys, every row
    ascending in image order, edge_rows == rows or 1 (every row counted on the one edge row);
    d_values: rows x nv keys of the same type; d_counts_out: rows x (nedges + 1) int32 / uint32
    words, which the call zeroes itself.  key: any of KEY.  NaNs are one value past every number and
    -0.0 < +0.0.  The call does not synchronise and reads nothing back, so it can be captured in a
    graph; a workspace is needed past bucket_counts_row_edges(key) edges only and is then, without
    `workspace`, taken from torch's allocator, which orders its reuse on the current stream only."""
    need = bucket_counts_workspace_bytes(edge_rows, nedges, key)
    wsb = 0
    if need or workspace is not None:
        workspace, wsb, _ = _workspace(workspace, lambda: need)
    opt = lambda t: None if t is None else _ptr(t)  # noqa: E731
    _check(lib.labsort_bucket_counts_device(opt(d_edges), edge_rows, nedges, opt(d_values), rows, nv, 1 if right else 0,
                                            KEY[key], opt(d_counts_out), opt(workspace), wsb, _stream(stream)),
           "bucket_counts_device")


def bincount_row_bins() -> int:
    """The most bins whose counters bincount_device keeps in LDS; past it every value is a global atomic."""
    return int(lib.labsort_bincount_row_bins())


def bincount_device(d_values, rows: int, nv: int, nbins: int, d_counts_out, key: str = "i32", stream=None) -> None:
    """d_counts_out[r][b], b < nbins = the number of values of row r equal to b; d_counts_out[r][nbins]
    = the number of its values outside [0, nbins).  d_values: rows x nv keys, key u32, i32, u64 or i64;
    d_counts_out: rows x (nbins + 1) int32 / uint32 words, which the call zeroes itself.  No workspace,
    no synchronisation, nothing read back."""
    opt = lambda t: None if t is None else _ptr(t)  # noqa: E731
    _check(lib.labsort_bincount_device(opt(d_values), rows, nv, nbins, KEY[key], opt(d_counts_out), _stream(stream)),
           "bincount_device")


def bucket_counts(input, boundaries, right: bool = False, workspace=None, stream=None):  # noqa: A002
    """The histogram of `input` over explicit edges: torch.bincount(ls.bucketize(input, boundaries,
    right), minlength=nedges + 1) per row, without the ranks ever being written.  input is 1-D or 2-D
    (rows x nv); boundaries is 1-D (nedges, shared by every row) or rows x nedges, ascending; both
    contiguous CUDA tensors of one dtype out of those searchsorted() takes.  Returns an int32 tensor of
    shape (nedges + 1,) or (rows, nedges + 1): count b is that of the values in (edge b-1, edge b]
    (right: [edge b-1, edge b)), count 0 lies below the first edge and count nedges past the last one, a
    NaN is one value past every number and -0.0 < +0.0.  torch.histogram differs: it counts in
    [edge b, edge b+1) with the last bin closed, drops what lies outside the edges and has no GPU form.
    Errors as searchsorted(): TypeError for a dtype that is not taken or differs between the two, a
    non-contiguous or a CPU tensor; ValueError for shapes that do not match; all before the device is
    touched."""
    import torch
    what = "bucket_counts"
    key = _search_tensor(what, "boundaries", boundaries)
    if _search_tensor(what, "input", input) != key:
        raise TypeError(f"{what}: boundaries is {boundaries.dtype}, input {input.dtype}: one dtype expected")
    named = [("boundaries", boundaries), ("input", input)]
    for name, t in named:
        if not t.is_contiguous():
            raise TypeError(f"{what}: {name}: a contiguous tensor expected")
    for name, t in named:
        if not t.is_cuda:
            raise TypeError(f"{what}: {name}: a CUDA tensor expected")
    if input.dim() not in (1, 2) or boundaries.dim() not in (1, 2):
        raise ValueError(f"{what}: a 1-D or 2-D input and 1-D or 2-D boundaries expected")
    rows, nv = (1, input.shape[0]) if input.dim() == 1 else input.shape
    if boundaries.dim() == 2 and (input.dim() != 2 or boundaries.shape[0] != rows):
        raise ValueError(f"{what}: boundaries of shape {tuple(boundaries.shape)} do not match the rows of the "
                         f"input's {tuple(input.shape)}")
    edge_rows, nedges = (rows if boundaries.dim() == 2 else 1), boundaries.shape[-1]
    out = torch.empty((nedges + 1,) if input.dim() == 1 else (rows, nedges + 1), dtype=torch.int32, device=input.device)
    if rows:  # (an empty tensor has no address to pass)
        bucket_counts_device(boundaries if nedges else None, edge_rows, nedges, input if nv else None, rows, nv, out,
                             right=right, key=key, workspace=workspace, stream=stream)
    return out


def bincount(input, nbins: int, stream=None):  # noqa: A002
    """Counts of the integers 0 .. nbins - 1 per row: input is a contiguous 1-D or 2-D CUDA tensor of
    int32, int64 or torch.uint32 / torch.uint64; the result is an int32 tensor of shape (nbins + 1,) or
    (rows, nbins + 1) whose last count is that of the values outside [0, nbins).  torch.bincount differs:
    its length is max(input) + 1 (at least minlength), which it reads back from the device, a negative
    value is an error there, and it takes one row only; here the length is the caller's, so the call
    neither synchronises nor depends on the data, and what does not fit is counted instead of refused."""
    import torch
    keys = {torch.int32: "i32", torch.int64: "i64"}
    for tname, key in (("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, tname):
            keys[getattr(torch, tname)] = key
    if not isinstance(input, torch.Tensor) or input.dtype not in keys:
        raise TypeError(f"bincount: input: int32, int64, uint32 or uint64 tensor expected, got {getattr(input, 'dtype', type(input))}")
    if not input.is_contiguous():
        raise TypeError("bincount: input: a contiguous tensor expected")
    if not input.is_cuda:
        raise TypeError("bincount: input: a CUDA tensor expected")
    if input.dim() not in (1, 2):
        raise ValueError("bincount: a 1-D or 2-D input expected")
    nbins = int(nbins)
    if nbins < 0:
        raise ValueError(f"bincount: nbins >= 0 expected, got {nbins}")
    rows, nv = (1, input.shape[0]) if input.dim() == 1 else input.shape
    out = torch.empty((nbins + 1,) if input.dim() == 1 else (rows, nbins + 1), dtype=torch.int32, device=input.device)
    if rows:
        bincount_device(input if nv else None, rows, nv, nbins, out, key=keys[input.dtype], stream=stream)
    return out


def key_order_bits(word: int, key: str = "u32") -> int:
    """The uint32 whose plain order is the key type's order of `word` (labsort_key_order_bits):
    u32 the word, i32 the word ^ 0x80000000, f32 the IEEE-754 order image (every NaN 0xFFFFFFFF)."""
    return int(lib.labsort_key_order_bits(int(word) & 0xFFFFFFFF, KEY[key]))


def key_from_order_bits(bits: int, key: str = "u32") -> int:
    """The inverse of key_order_bits (f32: the NaN image comes back as 0x7FFFFFFF)."""
    return int(lib.labsort_key_from_order_bits(int(bits) & 0xFFFFFFFF, KEY[key]))


def histogram(d_keys, n: int, d_hist, bits: int = 8, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_histogram(_ptr(d_keys), n, KEY[key], bits, _ptr(d_hist), _stream(stream)), "histogram")


def fill(d_out, n: int, seed: int, dist: str = "u32", param: int = 0, first: int = 0, stream=None) -> None:
    if dist == "reversed" and param == 0:
        param = first + n
    _check(lib.labsort_fill(_ptr(d_out), n, seed & (2**64 - 1), DIST[dist], param, first, _stream(stream)),
           "fill")


def upper_bound(d_sorted, n: int, d_values, nv: int, d_out, key: str = "u32", stream=None) -> None:
    """d_out[i] = number of keys <= d_values[i] in the sorted run (key order)."""
    _check(lib.labsort_upper_bound(_ptr(d_sorted) if n else 0, n, KEY[key], _ptr(d_values), nv, _ptr(d_out),
                                   _stream(stream)), "upper_bound")


def copy(d_in, d_out, n: int, stream=None) -> None:
    """d_out[0..n) = d_in[0..n) (32-bit words) by the library's streaming copy kernel."""
    _check(lib.labsort_copy(_ptr(d_in), _ptr(d_out), n, _stream(stream)), "copy")


def count_descents(d_keys, n: int, d_count, key: str = "u32", stream=None) -> None:
    _check(lib.labsort_count_descents(_ptr(d_keys), n, KEY[key], _ptr(d_count), _stream(stream)),
           "count_descents")


def timing_enable(on: bool = True) -> None:
    _check(lib.labsort_timing_enable(1 if on else 0), "timing_enable")


def timing_read(kclass: str) -> tuple[float, int]:
    ms, cnt = ctypes.c_double(0.0), ctypes.c_longlong(0)
    _check(lib.labsort_timing_read(KCLASS[kclass], ctypes.byref(ms), ctypes.byref(cnt)), "timing_read")
    return ms.value, cnt.value
