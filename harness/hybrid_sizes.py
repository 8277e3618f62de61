#!/usr/bin/env python3
"""The hybrid radix path's host gate by measurement (output kept as
profiles/hybrid_sizes.txt): labsort_sort_device, LABSORT_ALGO_RADIX, uniform uint32 keys, with
LABSORT_RADIX_HYBRID=0 (classic) and =2 (hybrid offered at any n) in turn, repetition by
repetition (device events around one call, one warm-up each); median [min, max] ms, and the
path the hybrid call took."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="", help="comma-separated n, each a Python expression (e.g. 3*2**26)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hybrid_sizes: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    sizes = [int(eval(x, {})) for x in a.sizes.split(",") if x] or [1 << 28]
    print(f"# radix sort of n uniform uint32 keys, classic (LABSORT_RADIX_HYBRID=0) against hybrid (=2), {a.reps} "
          f"alternating repetitions, ms: median [min, max]", file=out)
    os.environ["LABSORT_RADIX_IMPL"] = "onesweep"
    for n in sizes:
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        ls.fill(keys, n, seed=0x5EED0001, dist="u32")
        ko = torch.empty_like(keys)
        ws = torch.zeros(ls.workspace_bytes(n, "radix"), dtype=torch.uint8, device="cuda")
        t = {"0": [], "2": []}
        path = None
        for rep in range(a.reps + 1):  # (the first round warms up)
            for knob in t:
                os.environ["LABSORT_RADIX_HYBRID"] = knob
                ms = timed(lambda: ls.sort_device(keys, ko, n, key="u32", algo="radix", workspace=ws))
                if rep:
                    t[knob].append(ms)
                elif knob == "2":
                    ls.workspace_status(ws, n, "radix")
                    path = ls.radix_path(ws, n)
                    u = ko ^ -(1 << 31)  # unsigned order as int32 order
                    assert bool((u[1:] >= u[:-1]).all()), n
                    del u
        f = lambda ts: f"{statistics.median(ts):7.3f} [{min(ts):6.3f}, {max(ts):6.3f}]"
        print(f"n = {n:>10} ({n / (1 << 28):5.3f} x 2^28, {n >> 16} keys per bucket)  classic {f(t['0'])}  "
              f"hybrid {f(t['2'])}  path {path}  hybrid/classic {statistics.median(t['2']) / statistics.median(t['0']):.3f}",
              file=out)
        out.flush()
        del keys, ko, ws


if __name__ == "__main__":
    main()
