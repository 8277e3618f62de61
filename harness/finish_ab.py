#!/usr/bin/env python3
"""A/B of the hybrid radix sort's finish alone (output kept as
profiles/finish_ab.txt).

Several builds of liblabsort.so are loaded into one process.  For each size the same uniform
uint32 keys are sorted out of place by labsort_sort_device (LABSORT_ALGO_RADIX) with each build
in turn, repetition by repetition, with the library's timing hooks on; what is reported per
build is the `segsort` timing class of one sort (on the hybrid path that is the whole finish:
bucket offsets, class lists and the five class kernels) and the event time of the whole call,
ms, median [min, max] over the repetitions after the warm-ups.  Every build's first result is
compared with the first build's.

  python harness/finish_ab.py --lib parent=/path/liblabsort.so --lib new= --sizes 1,0.5,1.19

--lib NAME=PATH (an empty PATH: the package's own library); --sizes in units of 2^28 keys.  Sizes
other than 1 run under LABSORT_RADIX_HYBRID=2, which offers the hybrid path at any size."""
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

K_SEGSORT = ls.KCLASS["segsort"]
ALGO_RADIX = ls.ALGO["radix"]


def load(path):
    if not path:
        return ls.lib
    lib = ctypes.CDLL(path)
    for name in ("labsort_sort_device", "labsort_workspace_bytes", "labsort_workspace_status", "labsort_radix_path",
                 "labsort_timing_enable", "labsort_timing_read"):
        f, g = getattr(lib, name), getattr(ls.lib, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    return lib


def fmt(ts):
    return f"{statistics.median(ts):7.4f} [{min(ts):7.4f}, {max(ts):7.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH; empty PATH: the package's library")
    ap.add_argument("--sizes", default="1,0.5,1.19", help="comma-separated, in units of 2^28 keys")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("finish_ab: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    builds = {}
    for spec in a.lib or ["this="]:
        name, _, path = spec.partition("=")
        builds[name] = load(path)
    st = torch.cuda.current_stream().cuda_stream
    print(f"# finish A/B{': ' + a.note if a.note else ''}: {torch.cuda.get_device_name(0)}; {a.reps} alternating repetitions "
          f"after {a.warmup} warm-ups; ms per sort, median [min, max]", file=out)
    for size in [float(x) for x in a.sizes.split(",")]:
        n = int(size * (1 << 28))
        if size == 1.0:
            os.environ.pop("LABSORT_RADIX_HYBRID", None)
        else:
            os.environ["LABSORT_RADIX_HYBRID"] = "2"
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        ls.fill(keys, n, seed=0x5EED0001, dist="u32")
        res = torch.empty_like(keys)
        first = None
        nbytes = max(int(lib.labsort_workspace_bytes(n, ALGO_RADIX)) for lib in builds.values())
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        fin = {k: [] for k in builds}
        tot = {k: [] for k in builds}
        for rep in range(a.warmup + a.reps):
            for name, lib in builds.items():
                lib.labsort_timing_enable(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = lib.labsort_sort_device(keys.data_ptr(), res.data_ptr(), n, 0, ALGO_RADIX, ws.data_ptr(), nbytes, st)
                e1.record()
                e1.synchronize()
                if rc or lib.labsort_workspace_status(ws.data_ptr(), n, ALGO_RADIX, st):
                    sys.exit(f"finish_ab: {name}: the sort failed")
                ms, cnt = ctypes.c_double(0.0), ctypes.c_longlong(0)
                lib.labsort_timing_read(K_SEGSORT, ctypes.byref(ms), ctypes.byref(cnt))
                lib.labsort_timing_enable(0)
                if rep == 0:
                    if int(lib.labsort_radix_path(ws.data_ptr(), n, st)) != 1:
                        sys.exit(f"finish_ab: {name}: n = {n} did not take the hybrid path")
                    if first is None:
                        first = res.clone()
                    elif not torch.equal(res, first):
                        sys.exit(f"finish_ab: {name}: result differs from the first build's")
                if rep >= a.warmup:
                    fin[name].append(ms.value)
                    tot[name].append(e0.elapsed_time(e1))
        for name in builds:
            print(f"n = {size:g} x 2^28  {name:>8}  finish {fmt(fin[name])}   whole sort (timing hooks on) {fmt(tot[name])}", file=out)
        out.flush()
        del keys, res, ws, first


if __name__ == "__main__":
    main()
