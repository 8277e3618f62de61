#!/usr/bin/env python3
"""Searchsorted measurements on an MI355X.

Cases (--cases picks by name):
  buck255, buck4095   bucketize of 2^logn float32 standard normals on 255 / 4095 sorted boundaries (LDS
                      path, one shared sequence); beside it labsort_copy of the same bytes (the values
                      read, the ranks written)
  long_rand, long_sorted
                      2^(logn-2) uniform int32 values, as drawn and sorted, into a sorted int32 sequence
                      of 2^logn (long path), right side; also the library's older labsort_upper_bound
  rows_f32, rows_bf16 4096 rows: sequences of 4096, 4096 values each (a sequence per row, LDS path)
  long_i64            2^(logn-3) int64 values into 2^(logn-1) sorted int64 keys
  long_sorter         2^(logn-4) int32 values into an unsorted int32 sequence of 2^(logn-2) with the
                      sorter that orders it (long path)
Variants: new = labsort_searchsorted_device, torch = torch.searchsorted(out_int32=True, out=...) /
torch.bucketize, ub = labsort_upper_bound, copy = labsort_copy.  Every variant of a case is timed in
turn, repetition by repetition (device events around one call), after --warmup calls each; median
[min, max] ms.  The outputs of new, torch and ub are checked equal on the device before the timing.
Criterion per case and old route (the one of DESIGN.md §3.16): the slowest repetition of new below the
fastest of the old route."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

CASES = ["buck255", "buck4095", "long_rand", "long_sorted", "rows_f32", "rows_bf16", "long_i64", "long_sorter"]
KEY = {torch.int32: "i32", torch.float32: "f32", torch.bfloat16: "bf16", torch.int64: "i64"}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return t


def fmt(ts):
    return f"{statistics.median(ts):8.3f} [{min(ts):7.3f}, {max(ts):7.3f}]"


def rand_int(shape, bits, g):
    lo = torch.randint(0, 1 << 32, shape, dtype=torch.int64, device="cuda", generator=g)
    if bits == 32:
        return (lo - (1 << 31)).to(torch.int32)
    return (torch.randint(-(1 << 31), 1 << 31, shape, dtype=torch.int64, device="cuda", generator=g) << 32) | lo


def make(case, logn):
    """(sequence, values, sorter or None, right)"""
    g = torch.Generator(device="cuda").manual_seed(0x5EA7C4)
    n = 1 << logn
    if case.startswith("buck"):
        nb = int(case[4:])
        return torch.randn(nb, device="cuda", generator=g).sort().values, torch.randn(n, device="cuda", generator=g), None, False
    if case in ("long_rand", "long_sorted"):
        vals = rand_int((n >> 2,), 32, g)
        return rand_int((n,), 32, g).sort().values, vals.sort().values if case == "long_sorted" else vals, None, True
    if case.startswith("rows_"):
        dt = torch.float32 if case == "rows_f32" else torch.bfloat16
        seq = torch.randn((4096, 4096), device="cuda", generator=g).to(dt).sort(dim=-1).values.contiguous()
        return seq, torch.randn((4096, 4096), device="cuda", generator=g).to(dt), None, False
    if case == "long_i64":
        return rand_int((n >> 1,), 64, g).sort().values, rand_int((n >> 3,), 64, g), None, False
    assert case == "long_sorter", case
    seq = rand_int((n >> 2,), 32, g)
    return seq, rand_int((n >> 4,), 32, g), torch.argsort(seq, stable=True), True


def run_case(case, logn, reps, warmup, out):
    seq, vals, sorter, right = make(case, logn)
    key = KEY[seq.dtype]
    per_row = seq.dim() == 2
    seq_rows, cols = seq.shape if per_row else (1, seq.shape[0])
    rows, nv = vals.shape if per_row else (1, vals.numel())
    sorter32 = None if sorter is None else sorter.int()
    new = torch.empty(vals.shape, dtype=torch.int32, device="cuda")
    old = torch.empty_like(new)
    need = ls.searchsorted_workspace_bytes(seq_rows, cols, key)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") if need else None
    v = {"new": lambda: ls.searchsorted_device(seq, seq_rows, cols, vals, rows, nv, new, right=right, key=key, d_sorter=sorter32,
                                               workspace=ws)}
    if case.startswith("buck"):
        v["torch"] = lambda: torch.bucketize(vals, seq, out_int32=True, right=right, out=old)
        v["copy"] = lambda: ls.copy(vals, old, vals.numel())  # 4 bytes read and 4 written per value, as new moves
    else:
        v["torch"] = lambda: torch.searchsorted(seq, vals, out_int32=True, right=right, sorter=sorter, out=old)
    refused = None
    try:
        v["torch"]()
        torch.cuda.synchronize()
    except (RuntimeError, TypeError, NotImplementedError) as e:  # a dtype torch does not take: written down, not timed
        refused = str(e).splitlines()[0]
        del v["torch"]
    v["new"]()
    torch.cuda.synchronize()
    if refused is None:
        assert torch.equal(new, old), f"{case}: new differs from torch"
    if case in ("long_rand", "long_sorted"):
        ub = torch.empty_like(new)
        v["ub"] = lambda: ls.upper_bound(seq, cols, vals, nv, ub, key=key)
        v["ub"]()
        torch.cuda.synchronize()
        assert torch.equal(new, ub), f"{case}: new differs from labsort_upper_bound"
    t = alternate(v, reps, warmup)
    med = statistics.median
    esz = seq.element_size()
    print(f"{case}: {key} sequence {seq_rows} x {cols}, values {rows} x {nv}, right={right}, sorter={sorter is not None}, "
          f"{'long' if need else 'LDS'} path", file=out)
    for name, ts in t.items():
        print(f"    {name:<6}{fmt(ts)}", file=out)
    notes = [f"new {vals.numel() * (esz + 4) / med(t['new']) * 1e-9:.3f} TB/s of values read and ranks written"]
    if refused is not None:
        notes.append(f"torch refuses: {refused}")
    for route in ("torch", "ub"):
        if route in t:
            met = max(t["new"]) < min(t[route])
            notes.append(f"{route}/new {med(t[route]) / med(t['new']):.2f}, criterion vs {route} " + ("met" if met else "NOT met") +
                         f" (max new {max(t['new']):.3f}, min {route} {min(t[route]):.3f})")
    if "copy" in t:
        notes.append(f"new/copy {med(t['new']) / med(t['copy']):.2f}")
    print("    " + "; ".join(notes), file=out)
    out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("searchsorted_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    print(f"# searchsorted, {a.reps} alternating repetitions after {a.warmup} warm-up calls, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; chunk {ls.searchsorted_chunk_values()} values, "
          f"LDS path up to {ls.searchsorted_row_keys('f32')} 4-byte keys", file=out)
    for case in a.cases.split(","):
        run_case(case, a.logn, a.reps, a.warmup, out)
        torch.cuda.empty_cache()
