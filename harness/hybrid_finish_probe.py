#!/usr/bin/env python3
"""Price of the hybrid radix sort's finish on an MI355X (output kept as
profiles/hybrid_finish_probe.txt).

2^logn uniform uint32 keys are ordered by their top 16 bits only (torch.sort of key >> 16 and
a gather: what two LSD scatter passes on digits 2 and 3 leave), the 65537 bucket offsets are
built, and labsort_sort_segments_device sorts the buckets in place with max_segment_keys =
32768: each bucket is read once, sorted in LDS by its low two digits and written once.
  finish    that call, in place (the array is restored, untimed, before every repetition)
  copy      labsort_copy of the same keys: the 8 B/key floor
  sort      labsort_sort_device, LABSORT_ALGO_RADIX, of the unordered keys: the headline
Variants are timed in turn, repetition by repetition (device events around one call), after
one warm-up each; median [min, max] ms.

--libs LIB[,LIB...]: the same finish through alternative builds of liblabsort.so (make
EXTRA="-DLABSORT_SEG_BLOCK=.. -DLABSORT_SEG_BLOCK_KPT=.. -DLABSORT_SEG_BLOCK_WGS=.. -DLABSORT_SEG_BLOCK_WPE=.." BUILD=build_x
OUT=...: other shapes, so another upper edge, of the block class), alternating."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fmt(ts):
    return f"{statistics.median(ts):7.3f} [{min(ts):6.3f}, {max(ts):6.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", default="28", help="comma-separated log2 sizes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--libs", default="", help="comma-separated alternative builds of liblabsort.so")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hybrid_finish_probe: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    builds = {"this": ls.lib}
    for path in [p for p in a.libs.split(",") if p]:
        lib = ctypes.CDLL(path)
        lib.labsort_sort_segments_device.argtypes = ls.lib.labsort_sort_segments_device.argtypes
        lib.labsort_segment_class_edges.argtypes = ls.lib.labsort_segment_class_edges.argtypes
        builds[os.path.basename(path)] = lib
    st = torch.cuda.current_stream().cuda_stream
    print(f"# hybrid finish probe: buckets of the top 16 bits sorted in LDS, uint32 keys, {a.reps} alternating "
          f"repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    for name, lib in builds.items():
        e = (ctypes.c_size_t * 8)()
        k = lib.labsort_segment_class_edges(0, e, 8)
        print(f"# build {name}: class edges {[int(e[i]) for i in range(k)]}", file=out)
    nb = 1 << 16
    for logn in [int(x) for x in a.logn.split(",")]:
        n = 1 << logn
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        ls.fill(keys, n, seed=0x5EED0001, dist="u32")
        hi = (keys >> 16) & 0xFFFF
        src = keys[torch.sort(hi, stable=True).indices]
        cnt = torch.bincount(hi, minlength=nb)
        offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(cnt, 0)]).to(torch.int32)
        expect = torch.sort(keys ^ -(1 << 31)).values ^ -(1 << 31)
        del hi
        work, ko = torch.empty_like(src), torch.empty_like(src)
        ws = torch.zeros(ls.segments_workspace_bytes(n, nb, 32768), dtype=torch.uint8, device="cuda")
        rws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
        v = {}
        for name, lib in builds.items():
            v["finish/" + name] = (lambda lib=lib: lib.labsort_sort_segments_device(
                work.data_ptr(), work.data_ptr(), n, offs.data_ptr(), nb, 32768, 0, ws.data_ptr(), ws.numel(), st))
        v["copy"] = lambda: ls.copy(src, ko, n)
        v["sort"] = lambda: ls.sort_device(keys, ko, n, key="u32", algo="radix", workspace=rws)
        t = {k: [] for k in v}
        for rep in range(a.reps + 1):  # (the first round warms up)
            for k, fn in v.items():
                work.copy_(src)
                ms = timed(fn)
                if rep:
                    t[k].append(ms)
                elif k.startswith("finish/"):
                    ls.segments_workspace_status(ws)
                    assert torch.equal(work, expect), (logn, k)
        print(f"n = 2^{logn}  buckets {int(cnt.min())}..{int(cnt.max())} keys  " +
              "  ".join(f"{k} {fmt(ts)}" for k, ts in t.items()), file=out)
        out.flush()
        del keys, src, work, ko, ws, rws, expect


if __name__ == "__main__":
    main()
