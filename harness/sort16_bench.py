#!/usr/bin/env python3
"""Long 16-bit row sort measurements on an MI355X (output kept in
profiles/sort16.txt, part 2).

2^logn standard normals rounded to the type (bf16 / f16) as rows x cols -- one row of 2^logn keys,
rows of 131072, 151936 and 50257 keys -- sorted descending:
  new       labsort_sort16_device with positions: the two-pass radix on the 16-bit image
  new_k     the same without positions (the first two shapes)
  old       labsort_sort_rows_device with positions on the same buffers: the route to this result
            before (top-k's whole-row sort), code this path does not touch
  old_k     the same without positions
  torch     torch.sort(x, dim=-1, descending=True, stable=True): an outside comparator
  copy      labsort_copy of the input's bytes (one read and one write of the keys)
  ab:NAME   --ab NAME=/path/liblabsort.so: labsort_sort16_device of another build of the library
            (a chunk size or store form A/B, or the parent commit), with positions, in the same
            alternation; ab_k:NAME without.  With --ab every shape is run without positions too, and
            the line says whether new stays within the rule against the other build: its median
            exceeds the other's by at most the other's own max - min of the run.
Every variant of a shape is timed in turn, repetition by repetition (device events around one
call), after --warmup calls each (default one); median [min, max] ms over the repetitions.  B/key: the path's
24 (12 without positions) bytes per key over the time, in TB/s, beside the copy's rate (4 bytes per
key over its time).  `wins`: new's maximum lies below old's minimum, the condition for sort() to
route the shape to the new path."""
import argparse
import ctypes
import functools
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(1, 1 << 28, True), (2048, 131072, True), (1767, 151936, False), (5341, 50257, False)]  # (rows, cols, also keys only)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, warmup=1):
    """variants: {name: fn}.  warmup calls of each, then reps rounds over all of them."""
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


def med(ts):
    return statistics.median(ts)


def other_build(path):
    """labsort_sort16_device and its workspace size from another build of the library."""
    L = ctypes.CDLL(path)
    p, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.labsort_sort16_workspace_bytes.restype = sz
    L.labsort_sort16_workspace_bytes.argtypes = [sz, sz, i]
    L.labsort_sort16_chunk_keys.restype = sz
    L.labsort_sort16_device.argtypes = [p, sz, sz, i, i, p, p, p, sz, p]
    return L


def main(logn, reps, out, key, with_torch, shapes, ab, warmup=1):
    dt = DT[key]
    nmax = max(r * c for r, c, _ in shapes)
    x32 = torch.empty(nmax, dtype=torch.float32, device="cuda")
    x32.normal_(generator=torch.Generator(device="cuda").manual_seed(0x5167EED))
    xall = x32.to(dt)
    del x32
    print(f"# long 16-bit row sort, {key} keys (standard normal, rounded to the type), descending, {reps} alternating "
          f"repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; chunk {ls.sort16_chunk_keys()} keys"
          + "".join(f"; ab:{name} chunk {L.labsort_sort16_chunk_keys()} keys" for name, L in ab.items()), file=out)
    for rows, cols, keys_only in shapes:
        n = rows * cols
        x = xall[:n]
        ko, ko2 = torch.empty_like(x), torch.empty_like(x)
        io, io2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        ws = torch.full((ls.sort16_workspace_bytes(rows, cols, True),), 0xFF, dtype=torch.uint8, device="cuda")
        ws_o = torch.full((ls.sort_rows_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
        v = {"new": lambda: ls.sort16_device(x, rows, cols, ko, io, descending=True, key=key, workspace=ws)}
        if keys_only:
            v["new_k"] = lambda: ls.sort16_device(x, rows, cols, ko, None, descending=True, key=key, workspace=ws)
        v["old"] = lambda: ls.sort_rows_device(x, rows, cols, ko2, io2, descending=True, key=key, workspace=ws_o)
        if keys_only:
            v["old_k"] = lambda: ls.sort_rows_device(x, rows, cols, ko2, None, descending=True, key=key, workspace=ws_o)
        ab_ws = {}
        for name, L in ab.items():
            ab_ws[name] = torch.full((L.labsort_sort16_workspace_bytes(rows, cols, 1),), 0xFF, dtype=torch.uint8, device="cuda")

            def call(L=L, w=ab_ws[name], idx=True):
                rc = L.labsort_sort16_device(x.data_ptr(), rows, cols, 1, ls.KEY[key], ko.data_ptr(), io.data_ptr() if idx else None,
                                             w.data_ptr(), w.numel(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            v["ab:" + name] = call
            if keys_only:
                v["ab_k:" + name] = functools.partial(call, idx=False)
        if with_torch:
            v["torch"] = lambda: torch.sort(x.view(rows, cols), dim=-1, descending=True, stable=True)
        v["copy"] = lambda: ls.copy(x, ko2, n // 2)
        t = alternate(v, reps, warmup)
        # the result is the old route's, bit for bit (NaN-free inputs)
        v["old"]()
        ls.sort_rows_workspace_status(ws_o)
        for name in v:
            if name.startswith("new") or name.startswith("ab"):
                ko.zero_()
                io.zero_()
                v[name]()
                ls.sort16_workspace_status(ws)
                assert torch.equal(ko.view(torch.int16), ko2.view(torch.int16)), (name, rows, cols)
                assert name == "new_k" or name.startswith("ab_k:") or torch.equal(io, io2), (name, rows, cols)
        wins = ["new " + ("wins" if max(t["new"]) < min(t["old"]) else "DOES NOT WIN")]
        ratios = [f"old/new {med(t['old']) / med(t['new']):.2f}", f"new/copy {med(t['new']) / med(t['copy']):.2f}",
                  f"new {24 * n / med(t['new']) * 1e-9:.2f} TB/s at 24 B/key", f"copy {4 * n / med(t['copy']) * 1e-9:.2f} TB/s"]
        if keys_only:
            wins.append("new_k " + ("wins" if max(t["new_k"]) < min(t["old_k"]) else "DOES NOT WIN"))
            ratios += [f"old_k/new_k {med(t['old_k']) / med(t['new_k']):.2f}",
                       f"new_k {12 * n / med(t['new_k']) * 1e-9:.2f} TB/s at 12 B/key"]
        if with_torch:
            ratios.append(f"torch/new {med(t['torch']) / med(t['new']):.2f}")
        # against another build: within the rule when this build's median exceeds the other's by at most the
        # other's own max - min of the run
        for name in ab:
            for mine, theirs in [("new", "ab:" + name)] + ([("new_k", "ab_k:" + name)] if keys_only else []):
                over, spread = med(t[mine]) - med(t[theirs]), max(t[theirs]) - min(t[theirs])
                wins.append(f"{mine} - {theirs} {over:+.3f} (spread {spread:.3f}) {'within' if over <= spread else 'OVER'}")
        print(f"{key:<5}{rows:>6} x {cols:<10}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
              "  | " + "  ".join(ratios) + "  | " + ", ".join(wins), file=out)
        out.flush()
        del ws, ws_o, ab_ws, ko, ko2, io, io2, v


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28, help="keys per shape: the four shapes scaled to about 2^logn keys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--key", choices=list(DT), default="bf16")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--ab", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--warmup", type=int, default=1, help="calls of each variant before the timed ones")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sort16_bench: no GPU (no CPU fallback)")
    shapes = [(1, 1 << a.logn, k) if r == 1 else (max(1, (r << a.logn) >> 28), c, k) for r, c, k in SHAPES]
    ab = {s.split("=", 1)[0]: other_build(s.split("=", 1)[1]) for s in a.ab}
    if ab:
        shapes = [(r, c, True) for r, c, _ in shapes]
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.logn, a.reps, out, a.key, not a.no_torch, shapes, ab, a.warmup)
