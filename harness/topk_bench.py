#!/usr/bin/env python3
"""Top-k selection measurements on an MI355X (output kept as
profiles/topk_bench.txt).

int32 keys (--key i32), 2^28 in all, as rows x cols, smallest k with positions, on uniform keys and
on keys % 1000; or float32 keys (--key f32), standard normal, on which the torch comparator runs
as it would for a caller with float data:
  topk      labsort_topk_device
  fullsort  what a caller could do before it: one row, labsort_sort_pairs_device of (key, iota);
            several rows, labsort_sort_segments_pairs_device with max_segment_keys = cols
  copy      labsort_copy of the same keys (one read and one write: a read costs half of it)
  torch     torch.topk(x, k, largest=False, sorted=True): an outside comparator, recorded only
Every variant of a shape is timed in turn, repetition by repetition (device events around one
call), after one warm-up each; median [min, max] ms over the repetitions.

--key bf16 / f16 (output kept in profiles/f16_keys.txt): standard-normal values
rounded to the type, on the three shapes 1 x n k 1024, n/2^16 x 2^16 k 64, n/4096 x 4096 k 8:
  topk      labsort_topk_device on the 16-bit tensor
  f32       the float32 call on the same values widened beforehand: the yardstick
  widen     x.float(), the pass a caller without 16-bit keys pays before it
  torch     torch.topk on the 16-bit tensor
  copy      labsort_copy of the input's bytes
--parent PATH (any --key): the same top-k call through another build of liblabsort.so, alternating
with this one on the same buffers after --warmup calls of each (the regression check of a change to
topk.hip); int32 keys also on one row of keys % 1000, which never narrows.  Outputs must be equal word
for word.  A shape is within the rule when this build's median exceeds the parent's by at most the
parent's own max - min of the run.
--largest: the k largest, as torch.topk's default.

--sweep: the large-k threshold.  One row of 2^logn keys, k from 2^10 up to the whole row, with the
path forced either way (LABSORT_TOPK_PATH=select / sort, read at every call), alternating."""
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


def forced(path, fn):
    def f():
        os.environ["LABSORT_TOPK_PATH"] = path
        try:
            fn()
        finally:
            del os.environ["LABSORT_TOPK_PATH"]
    return f


def check(keys, rows, cols, k, ko, io):
    """Keys against torch.sort; positions by gathering (torch's tie order is its own)."""
    x = keys.view(rows, cols)
    exp = torch.sort(x, dim=1, stable=True).values[:, :k]
    assert torch.equal(ko.view(rows, k), exp), (rows, cols, k)
    assert torch.equal(torch.gather(x, 1, io.view(rows, k).long()), exp), (rows, cols, k)
    del exp


def parent_topk(path):
    """labsort_topk_device of another build of the library (same signature), as a callable."""
    import ctypes
    L = ctypes.CDLL(path)
    p, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.labsort_topk_device.argtypes = [p, sz, sz, sz, i, i, p, p, p, sz, p]

    def call(keys, rows, cols, k, ko, io, largest, key, ws):
        st = L.labsort_topk_device(keys.data_ptr(), rows, cols, k, 1 if largest else 0, ls.KEY[key], ko.data_ptr(), io.data_ptr(),
                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
    return call


def f16_main(logn, reps, out, with_torch, key, largest):
    """16-bit keys against the float32 call on the same values (module docstring)."""
    n = 1 << logn
    dt = torch.bfloat16 if key == "bf16" else torch.float16
    x32 = torch.empty(n, dtype=torch.float32, device="cuda")
    x32.normal_(generator=torch.Generator(device="cuda").manual_seed(0x70C0EED))
    x = x32.to(dt)       # rounded to the type
    x32.copy_(x)         # the same values, widened beforehand
    cp = torch.empty_like(x)
    print(f"# top-k, {key} keys (standard normal, rounded to the type), {'largest' if largest else 'smallest'} k with positions, "
          f"n = 2^{logn}, {reps} alternating repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    for rows, cols, k in [(1, n, 1024), (n >> 16, 1 << 16, 64), (n >> 12, 4096, 8)]:
        ko = torch.empty(rows * k, dtype=dt, device="cuda")
        ko32 = torch.empty(rows * k, dtype=torch.float32, device="cuda")
        io = torch.empty(rows * k, dtype=torch.int32, device="cuda")
        io32 = torch.empty_like(io)
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
        v = {"topk": lambda: ls.topk_device(x, rows, cols, k, ko, io, largest=largest, key=key, workspace=ws),
             "f32": lambda: ls.topk_device(x32, rows, cols, k, ko32, io32, largest=largest, key="f32", workspace=ws),
             "widen": lambda: x.float(),
             "copy": lambda: ls.copy(x, cp, n // 2)}
        if with_torch:
            v["torch"] = lambda: torch.topk(x.view(rows, cols), k, dim=1, largest=largest, sorted=True)
        t = alternate(v, reps)
        ko.zero_()
        v["topk"]()
        ls.topk_workspace_status(ws)
        v["f32"]()
        ls.topk_workspace_status(ws)
        # the same values and, the order maps agreeing, the same positions as the float32 call
        assert torch.equal(ko.float(), ko32) and torch.equal(io, io32), (rows, cols, k)
        assert torch.equal(torch.gather(x.view(rows, cols), 1, io.view(rows, k).long()), ko.view(rows, k)), (rows, cols, k)
        path = "short" if cols <= ls.segment_pair_tile_keys() else ("sort" if k * ls.TOPK_SORT_DIV > cols else "select")
        print(f"{key:<6}{rows:>6} x {cols:<10} k {k:<6} {path:<7}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
              f"  topk/f32 {med(t['topk']) / med(t['f32']):.3f}  topk/(f32+widen) {med(t['topk']) / (med(t['f32']) + med(t['widen'])):.3f}"
              f"  topk/copy {med(t['topk']) / med(t['copy']):.2f}", file=out)
        out.flush()
        del ws, ko, ko32, io, io32


def parent_main(logn, reps, out, key, largest, path, warmup):
    """This build against another one (--parent) on the 16-bit shapes."""
    n = 1 << logn
    other = parent_topk(path)
    dt = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[key]
    keys = torch.empty(n, dtype=torch.int32 if key == "i32" else torch.float32, device="cuda")
    print(f"# top-k, {key} keys, {'largest' if largest else 'smallest'} k with positions, n = 2^{logn}: this build (new) against "
          f"{path} (parent), {warmup} warm-up calls, {reps} alternating repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    shapes = [("", 1, n, 1024), ("", n >> 16, 1 << 16, 64), ("", n >> 12, 4096, 8)]
    if key == "i32":
        shapes.append(("mod1000", 1, n, 1024))
    filled = None
    for dist, rows, cols, k in shapes:
        if dist != filled:
            if key == "i32":
                ls.fill(keys, n, seed=0x70C0EED, dist=dist or "u32")
            else:  # standard normal, for the 16-bit types rounded to the type
                keys.normal_(generator=torch.Generator(device="cuda").manual_seed(0x70C0EED))
            x = keys if keys.dtype == dt else keys.to(dt)
            filled = dist
        ko, ko2 = (torch.empty(rows * k, dtype=dt, device="cuda") for _ in range(2))
        io, io2 = (torch.empty(rows * k, dtype=torch.int32, device="cuda") for _ in range(2))
        ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
        v = {"new": lambda: ls.topk_device(x, rows, cols, k, ko, io, largest=largest, key=key, workspace=ws),
             "parent": lambda: other(x, rows, cols, k, ko2, io2, largest, key, ws)}
        t = alternate(v, reps, warmup)
        torch.cuda.synchronize()
        bits = torch.int32 if dt.itemsize == 4 else torch.int16
        assert torch.equal(ko.view(bits), ko2.view(bits)) and torch.equal(io, io2), (rows, cols, k)
        over, spread = med(t["new"]) - med(t["parent"]), max(t["parent"]) - min(t["parent"])
        print(f"{key:<6}{dist:<8}{rows:>6} x {cols:<10} k {k:<6}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
              f"  new/parent {med(t['new']) / med(t['parent']):.3f}  new - parent {over:+.3f}  parent's spread {spread:.3f}  "
              f"{'within' if over <= spread else 'OVER'}", file=out)
        out.flush()
        del ws, ko, ko2, io, io2


def shapes_main(logn, reps, out, with_torch, key="i32"):
    n = 1 << logn
    keys = torch.empty(n, dtype=torch.float32 if key == "f32" else torch.int32, device="cuda")
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    so, sv = torch.empty_like(keys), torch.empty_like(iota)
    print(f"# top-k, {'float32' if key == 'f32' else 'int32'} keys, smallest k with positions, n = 2^{logn}, {reps} alternating repetitions, "
          "ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    shapes = [(1, n, 1), (1, n, 1024), (1, n, min(1 << 20, n)), (n >> 16, 1 << 16, 64), (n >> 12, 4096, 8)]
    for dist in (("normal",) if key == "f32" else ("u32", "mod1000")):
        if key == "f32":
            keys.normal_(generator=torch.Generator(device="cuda").manual_seed(0x70C0EED))
        else:
            ls.fill(keys, n, seed=0x70C0EED, dist=dist)
        torch.cuda.synchronize()
        for rows, cols, k in shapes:
            ko = torch.empty(rows * k, dtype=keys.dtype, device="cuda")
            io = torch.empty(rows * k, dtype=torch.int32, device="cuda")
            ws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
            v = {"topk": lambda: ls.topk_device(keys, rows, cols, k, ko, io, key=key, workspace=ws)}
            if rows == 1:
                ws_f = torch.empty(ls.pairs_workspace_bytes(n, "auto"), dtype=torch.uint8, device="cuda")
                v["fullsort"] = lambda: ls.sort_pairs_device(keys, iota, so, sv, n, key=key, algo="auto", workspace=ws_f)
            else:
                offs = ls.row_offsets(rows, cols)
                ws_f = torch.empty(ls.segments_workspace_bytes(n, rows, cols, True), dtype=torch.uint8, device="cuda")
                v["fullsort"] = lambda: ls.sort_segments_pairs_device(keys, iota, so, sv, n, offs, rows, cols, key=key,
                                                                      workspace=ws_f)
            v["copy"] = lambda: ls.copy(keys, so, n)
            if with_torch:
                v["torch"] = lambda: torch.topk(keys.view(rows, cols), k, dim=1, largest=False, sorted=True)
            t = alternate(v, reps)
            ko.zero_()
            v["topk"]()
            ls.topk_workspace_status(ws)
            check(keys, rows, cols, k, ko, io)
            path = "short" if cols <= ls.segment_pair_tile_keys() else ("sort" if k * ls.TOPK_SORT_DIV > cols else "select")
            print(f"{dist:<8}{rows:>6} x {cols:<10} k {k:<8} {path:<7}" +
                  "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
                  f"  topk/fullsort {med(t['topk']) / med(t['fullsort']):.3f}  topk/copy {med(t['topk']) / med(t['copy']):.2f}",
                  file=out)
            out.flush()
            del ws, ws_f, ko, io


def sweep_main(logn, reps, out):
    n = 1 << logn
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    print(f"# large-k sweep, one row of 2^{logn} int32 keys, path forced, {reps} alternating repetitions, "
          "ms: median [min, max]", file=out)
    for dist in ("u32", "mod1000"):
        ls.fill(keys, n, seed=0x70C0EED, dist=dist)
        torch.cuda.synchronize()
        for k in [1 << lk for lk in range(10, logn - 2, 2)] + [n // 8, n // 4, 3 * (n // 8), n // 2, 3 * (n // 4), n]:
            ko = torch.empty(k, dtype=torch.int32, device="cuda")
            io = torch.empty(k, dtype=torch.int32, device="cuda")
            v, wss = {}, {}
            for path in ("select", "sort"):
                os.environ["LABSORT_TOPK_PATH"] = path
                wss[path] = torch.empty(ls.topk_workspace_bytes(1, n, k), dtype=torch.uint8, device="cuda")
                del os.environ["LABSORT_TOPK_PATH"]
                v[path] = forced(path, lambda w=wss[path]: ls.topk_device(keys, 1, n, k, ko, io, key="i32", workspace=w))
            t = alternate(v, reps)
            print(f"{dist:<8}k {k:<10} k/cols {k / n:<10.6f}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
                  f"  select/sort {med(t['select']) / med(t['sort']):.3f}", file=out)
            out.flush()
            del wss, ko, io


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--key", choices=["i32", "f32", "bf16", "f16"], default="i32",
                    help="f32: standard-normal float32 keys; bf16 / f16: the same rounded to the type, against the f32 call")
    ap.add_argument("--largest", action="store_true", help="bf16 / f16 and --parent runs: the k largest")
    ap.add_argument("--parent", default="", help="another build of liblabsort.so to alternate with")
    ap.add_argument("--warmup", type=int, default=1, help="--parent runs: calls of each build before the timed ones")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    if a.sweep:
        sweep_main(a.logn, a.reps, out)
    elif a.parent:
        parent_main(a.logn, a.reps, out, a.key, a.largest, a.parent, a.warmup)
    elif a.key in ("bf16", "f16"):
        f16_main(a.logn, a.reps, out, not a.no_torch, a.key, a.largest)
    else:
        shapes_main(a.logn, a.reps, out, not a.no_torch, a.key)
