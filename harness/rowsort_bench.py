#!/usr/bin/env python3
"""Dense row sort measurements on an MI355X (output kept in profiles/rowsort.txt,
part 2).

2^logn keys as rows x cols, cols in 256 / 4096 / 16384 (and 32768 where the LDS path takes it:
16-bit keys, 32-bit keys without positions), standard normals rounded to the type (--key f32 /
bf16 / f16) or uniform int32 (--key i32), ascending and descending:
  sort      labsort_sort_rows_device with positions (the grid form the library chooses per class)
  sort_pr   the same with one wave / workgroup per row, sort_fx with the fixed grid and a row loop
            (LABSORT_ROWSORT_GRID=rows / fixed, read at every call): the A/B of the grid form
  keys      labsort_sort_rows_device without positions
  topk      labsort_topk_device with k = cols and positions: the route to this result before
  topk_k    the same without positions (the yardstick of `keys`)
  segpairs  32-bit keys: labsort_sort_segments_pairs_device on (key, iota) with uniform offsets
            (ascending only: it has no other direction; timed in both tables all the same)
  torch     torch.sort(x, dim=1, descending=..., stable=True): an outside comparator, recorded only
  copy      labsort_copy of the input's bytes (one read and one write of the keys)
Every variant of a shape is timed in turn, repetition by repetition (device events around one
call), after one warm-up each; median [min, max] ms over the repetitions.  `wins`: the call's
maximum lies below the minimum of each library yardstick (topk and segpairs for sort, topk_k for
keys)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

DT = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps):
    """variants: {name: fn}.  One warm-up each, then reps rounds over all of them."""
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


def grid_form(form, fn):
    def f():
        os.environ["LABSORT_ROWSORT_GRID"] = form
        try:
            fn()
        finally:
            del os.environ["LABSORT_ROWSORT_GRID"]
    return f


def main(logn, reps, out, key, with_torch, shapes):
    n = 1 << logn
    dt = DT[key]
    k16 = key in ("bf16", "f16")
    if key == "i32":
        x = torch.empty(n, dtype=dt, device="cuda")
        ls.fill(x, n, seed=0x70C0EED, dist="u32")
    else:
        x32 = torch.empty(n, dtype=torch.float32, device="cuda")
        x32.normal_(generator=torch.Generator(device="cuda").manual_seed(0x70C0EED))
        x = x32.to(dt)
        del x32
    ko, ko2 = torch.empty_like(x), torch.empty_like(x)
    io, io2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    iota = None if k16 else torch.arange(n, dtype=torch.int32, device="cuda")
    print(f"# row sort, {key} keys ({'uniform' if key == 'i32' else 'standard normal, rounded to the type'}), n = 2^{logn}, "
          f"{reps} alternating repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    TP, TK = ls.segment_pair_tile_keys(), ls.segment_tile_keys()
    for cols in shapes:
        rows = n // cols
        idx_lds = cols <= (TK if k16 else TP)  # the call with positions takes the LDS path
        if cols > TK:
            continue
        ws = torch.full((ls.sort_rows_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
        ws_t = torch.full((ls.topk_workspace_bytes(rows, cols, cols),), 0xFF, dtype=torch.uint8, device="cuda")
        for desc in (False, True):
            v = {}
            if idx_lds:
                v["sort"] = lambda: ls.sort_rows_device(x, rows, cols, ko, io, descending=desc, key=key, workspace=ws)
                v["sort_pr"] = grid_form("rows", v["sort"])
                v["sort_fx"] = grid_form("fixed", v["sort"])
            v["keys"] = lambda: ls.sort_rows_device(x, rows, cols, ko, None, descending=desc, key=key, workspace=ws)
            v["topk"] = lambda: ls.topk_device(x, rows, cols, cols, ko2, io2, largest=desc, key=key, workspace=ws_t)
            v["topk_k"] = lambda: ls.topk_device(x, rows, cols, cols, ko2, None, largest=desc, key=key, workspace=ws_t)
            if not k16 and cols <= TP:
                offs = ls.row_offsets(rows, cols)
                ws_s = torch.empty(ls.segments_workspace_bytes(n, rows, cols, True), dtype=torch.uint8, device="cuda")
                v["segpairs"] = lambda: ls.sort_segments_pairs_device(x, iota, ko2, io2, n, offs, rows, cols, key=key, workspace=ws_s)
            if with_torch:
                v["torch"] = lambda: torch.sort(x.view(rows, cols), dim=1, descending=desc, stable=True)
            v["copy"] = lambda: ls.copy(x, ko2, n // 2 if k16 else n)
            t = alternate(v, reps)
            # the result is top-k's, bit for bit (NaN-free inputs)
            v["topk"]()
            ls.topk_workspace_status(ws_t)
            for name in ("sort", "sort_pr", "sort_fx", "keys"):
                if name in v:
                    ko.zero_()
                    io.zero_()
                    v[name]()
                    ls.sort_rows_workspace_status(ws)
                    assert torch.equal(ko.view(torch.int16), ko2.view(torch.int16)), (name, rows, cols, desc)
                    assert name == "keys" or torch.equal(io, io2), (name, rows, cols, desc)
            wins = []
            if "sort" in t:
                yard = [y for y in ("topk", "segpairs") if y in t]
                wins.append("sort " + ("wins" if all(max(t["sort"]) < min(t[y]) for y in yard) else "DOES NOT WIN"))
            wins.append("keys " + ("wins" if max(t["keys"]) < min(t["topk_k"]) else "DOES NOT WIN"))
            ratios = []
            if "sort" in t:
                ratios += [f"topk/sort {med(t['topk']) / med(t['sort']):.2f}", f"sort/copy {med(t['sort']) / med(t['copy']):.2f}",
                           f"sort_pr/sort_fx {med(t['sort_pr']) / med(t['sort_fx']):.3f}"]
                if "segpairs" in t:
                    ratios.append(f"segpairs/sort {med(t['segpairs']) / med(t['sort']):.2f}")
            ratios += [f"topk_k/keys {med(t['topk_k']) / med(t['keys']):.2f}", f"keys/copy {med(t['keys']) / med(t['copy']):.2f}"]
            print(f"{key:<5}{rows:>8} x {cols:<6} {'desc' if desc else 'asc ':<5}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
                  "  | " + "  ".join(ratios) + "  | " + ", ".join(wins), file=out)
            out.flush()
        del ws, ws_t


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--key", choices=list(DT), default="bf16")
    ap.add_argument("--cols", type=int, nargs="*", default=[256, 4096, 16384, 32768])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rowsort_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.logn, a.reps, out, a.key, not a.no_torch, a.cols)
