#!/usr/bin/env python3
"""A/B of the LDS class kernels against another build of liblabsort.so, usually the parent
commit's (output kept in profiles/lds_classes.txt, part 3).

2^logn keys as rows x cols, one shape per class (cols 256 / 512 / 1024 / 4096 / 16384), int32
(uniform) and float32 (standard normal) keys, through both families:
  rows      labsort_sort_rows_device, keys only and with positions
  segments  labsort_sort_segments_device / labsort_sort_segments_pairs_device with
            max_segment_keys = cols (the LDS path), keys only and with payloads
and bfloat16 rows with positions at 1024 and 32768 columns (the packed 16-bit kernels).  Both
builds are loaded in this process and called alternating, repetition by repetition, after two
warm-up calls each (device events around one call); ms, median [min, max].  `ok`: this build's
median minus the other's is no more than the other's max - min (the project's rule, §3.8).
Both builds' outputs are compared word for word, once per shape."""
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

DT = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fmt(ts):
    return f"{statistics.median(ts):7.4f} [{min(ts):7.4f}, {max(ts):7.4f}]"


def entry(lib, name):
    """The C entry `name` of a build, with the module's argument types."""
    f = getattr(lib, name)
    f.argtypes = getattr(ls.lib, name).argtypes
    return f


def main(logn, reps, other, out, only):
    n = 1 << logn
    builds = {"other": ctypes.CDLL(other), "this": ls.lib}
    st = torch.cuda.current_stream().cuda_stream
    print(f"# LDS class kernels, n = 2^{logn}, 2 warm-up calls and {reps} alternating repetitions per build, ms: median [min, max]",
          file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; this: {ls.version()}; other: {other}", file=out)
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    shapes = [(key, cols) for key in ("i32", "f32") for cols in (256, 512, 1024, 4096, 16384)] + [("bf16", 1024), ("bf16", 32768)]
    data = {}
    for key, cols in shapes:
        if only and key not in only:
            continue
        if key not in data:
            data.clear()
            if key == "i32":
                x = torch.empty(n, dtype=torch.int32, device="cuda")
                ls.fill(x, n, seed=0x1D5C1A55, dist="u32")
            else:
                x = torch.empty(n, dtype=torch.float32, device="cuda")
                x.normal_(generator=torch.Generator(device="cuda").manual_seed(0x1D5C1A55))
                x = x.to(DT[key])
            data[key] = x
        x = data[key]
        rows = n // cols
        kt = ls.KEY[key]
        offs = ls.row_offsets(rows, cols)
        ko = {b: torch.empty_like(x) for b in builds}
        vo = {b: torch.empty(n, dtype=torch.int32, device="cuda") for b in builds}
        cases = {}
        ws_r = torch.zeros(ls.sort_rows_workspace_bytes(rows, cols), dtype=torch.uint8, device="cuda")
        for b, lib in builds.items():
            f = entry(lib, "labsort_sort_rows_device")
            if key != "bf16":
                cases.setdefault("rows, keys only", {})[b] = (
                    lambda f=f, b=b: f(x.data_ptr(), rows, cols, 0, kt, ko[b].data_ptr(), None, ws_r.data_ptr(), ws_r.numel(), st))
            cases.setdefault("rows, positions", {})[b] = (
                lambda f=f, b=b: f(x.data_ptr(), rows, cols, 0, kt, ko[b].data_ptr(), vo[b].data_ptr(), ws_r.data_ptr(), ws_r.numel(), st))
        if key != "bf16":
            ws_k = torch.zeros(ls.segments_workspace_bytes(n, rows, cols, False), dtype=torch.uint8, device="cuda")
            ws_p = torch.zeros(ls.segments_workspace_bytes(n, rows, cols, True), dtype=torch.uint8, device="cuda")
            for b, lib in builds.items():
                f = entry(lib, "labsort_sort_segments_device")
                g = entry(lib, "labsort_sort_segments_pairs_device")
                cases.setdefault("segments, keys only", {})[b] = (
                    lambda f=f, b=b: f(x.data_ptr(), ko[b].data_ptr(), n, offs.data_ptr(), rows, cols, kt, ws_k.data_ptr(), ws_k.numel(), st))
                cases.setdefault("segments, payloads", {})[b] = (
                    lambda g=g, b=b: g(x.data_ptr(), vals.data_ptr(), ko[b].data_ptr(), vo[b].data_ptr(), n, offs.data_ptr(), rows, cols,
                                       kt, ws_p.data_ptr(), ws_p.numel(), st))
        for name, v in cases.items():
            for b in builds:
                ko[b].zero_()
                vo[b].zero_()
            for _ in range(2):
                for fn in v.values():
                    if fn() != 0:
                        sys.exit(f"lds_classes_ab: {key} {cols} {name}: the call returned an error")
            torch.cuda.synchronize()
            same = torch.equal(ko["this"].view(torch.uint8), ko["other"].view(torch.uint8))
            if "keys only" not in name:
                same = same and torch.equal(vo["this"], vo["other"])
            t = {b: [] for b in builds}
            for _ in range(reps):
                for b, fn in v.items():
                    t[b].append(timed(fn))
            d = statistics.median(t["this"]) - statistics.median(t["other"])
            spread = max(t["other"]) - min(t["other"])
            print(f"{key:<5}{rows:>8} x {cols:<6} {name:<20} other {fmt(t['other'])}  this {fmt(t['this'])}  "
                  f"diff {d:+.4f}  other's spread {spread:.4f}  {'ok' if d <= spread else 'SLOWER'}  "
                  f"outputs {'equal' if same else 'DIFFER'}", file=out)
            out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the other build of liblabsort.so")
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--key", nargs="*", default=[], help="only these key types (i32 f32 bf16)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lds_classes_ab: no GPU (no CPU fallback)")
    main(a.logn, a.reps, a.other, open(a.out, "a") if a.out else sys.stdout, a.key)
