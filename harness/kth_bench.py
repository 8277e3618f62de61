#!/usr/bin/env python3
"""k-th key selection measurements on an MI355X (output kept in profiles/kth.txt).

2^logn standard normals as rows x cols -- one row, rows of 2^16, 151936 and 4096 keys -- as float32,
rounded to bfloat16, or in fixed point as int32 (round(x * 2^28): the concentrated top byte stays);
the k-th smallest key of every row with its position, for k = 1, 1024, cols // 2 and a random k per row:
  new     labsort_kth_device with positions (a host k, or d_k for the k per row)
  old     the route to this result before, on the same build and buffers: labsort_topk_device(k) and
          its last column where k <= cols / 4 (old:topk); else every row sorted with positions and
          column k - 1 (old:rows labsort_sort_rows_device, old:s16 labsort_sort16_device for bfloat16);
          for a k per row always the whole-row sort
  torch   torch.kthvalue(x, k, dim=1) where torch takes the dtype and the shape (one k only)
  copy    labsort_copy of the input's bytes (one read and one write of the keys)
Every variant of a case is timed in turn, repetition by repetition (device events around one call),
after --warmup calls each; ms: median [min, max] over the repetitions.  `wins`: new's maximum lies
below old's minimum.  Before the timing new's keys and positions are compared with old's column."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

DT = {"i32": torch.int32, "f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [(1, 1 << 28), (4096, 1 << 16), (1767, 151936), (1 << 16, 4096)]


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


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def make_keys(key, n):
    x32 = torch.empty(n, dtype=torch.float32, device="cuda")
    x32.normal_(generator=torch.Generator(device="cuda").manual_seed(0x4B7EED))
    if key == "f32":
        return x32
    if key == "bf16":
        return x32.to(torch.bfloat16)
    return (x32.double() * float(1 << 28)).round().clamp(-(2**31), 2**31 - 1).to(torch.int32)


def main(reps, out, keys, shapes, with_torch, warmup):
    print(f"# k-th smallest key per row with its position, standard-normal keys, {reps} alternating repetitions, "
          f"ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; one launch up to {ls.kth_row_keys()} keys per row; "
          f"library {os.path.basename(ls.LIB_PATH)}", file=out)
    for key in keys:
        xall = make_keys(key, max(r * c for r, c in shapes))
        esz = xall.element_size()
        for rows, cols in shapes:
            n = rows * cols
            x = xall[:n]
            ko = torch.empty(rows, dtype=xall.dtype, device="cuda")
            io = torch.empty(rows, dtype=torch.int32, device="cuda")
            ws = torch.full((ls.kth_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
            cdst = torch.empty(n * esz // 4, dtype=torch.int32, device="cuda")
            # the whole-row sort of the route before: its outputs and workspace
            use16 = key == "bf16"
            sk = torch.empty(n, dtype=xall.dtype, device="cuda")
            si = torch.empty(n, dtype=torch.int32, device="cuda")
            sws = torch.full(((ls.sort16_workspace_bytes(rows, cols, True) if use16 else ls.sort_rows_workspace_bytes(rows, cols)),),
                             0xFF, dtype=torch.uint8, device="cuda")

            def sort_rows():
                if use16:
                    ls.sort16_device(x, rows, cols, sk, si, descending=False, key=key, workspace=sws)
                else:
                    ls.sort_rows_device(x, rows, cols, sk, si, descending=False, key=key, workspace=sws)
            sort_rows()
            torch.cuda.synchronize()
            g = torch.Generator(device="cuda").manual_seed(0x4B7EED + cols)
            kper = torch.randint(1, cols + 1, (rows,), generator=g, device="cuda", dtype=torch.int32)
            for label, k in (("k=1", 1), ("k=1024", 1024), ("k=cols/2", cols // 2), ("k per row", kper)):
                per_row = not isinstance(k, int)
                v = {"new": lambda k=k: ls.kth_device(x, rows, cols, k, ko, io, key=key, workspace=ws)}
                if not per_row and k * 4 <= cols:
                    old = "old:topk"
                    tk = torch.empty(rows * k, dtype=xall.dtype, device="cuda")
                    ti = torch.empty(rows * k, dtype=torch.int32, device="cuda")
                    tws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")
                    v[old] = lambda k=k, tk=tk, ti=ti, tws=tws: ls.topk_device(x, rows, cols, k, tk, ti, largest=False, key=key, workspace=tws)
                else:
                    old = "old:s16" if use16 else "old:rows"
                    v[old] = sort_rows
                if with_torch and not per_row:
                    try:
                        torch.kthvalue(x.view(rows, cols), k, dim=1)
                        torch.cuda.synchronize()
                        v["torch"] = lambda k=k: torch.kthvalue(x.view(rows, cols), k, dim=1)
                    except Exception as err:  # (a dtype or a shape torch does not take)
                        print(f"# torch.kthvalue {key} {rows} x {cols} {label}: {type(err).__name__}", file=out)
                v["copy"] = lambda: ls.copy(x, cdst, n * esz // 4)
                # the result is the route before's, bit for bit (NaN-free input)
                ko.zero_()
                io.zero_()
                v["new"]()
                ls.kth_workspace_status(ws)
                v[old]()
                torch.cuda.synchronize()
                r = torch.arange(rows, device="cuda")
                kk = (k.long() if per_row else torch.full((rows,), k, device="cuda")) - 1
                if old == "old:topk":
                    ek, ei = tk.view(rows, k)[:, k - 1], ti.view(rows, k)[:, k - 1]
                else:
                    ek, ei = sk.view(rows, cols)[r, kk], si.view(rows, cols)[r, kk]
                assert torch.equal(bits(ko), bits(ek.contiguous())) and torch.equal(io, ei.contiguous()), (key, rows, cols, label)
                t = alternate(v, reps, warmup)
                med = {name: statistics.median(ts) for name, ts in t.items()}
                verdict = "new wins" if max(t["new"]) < min(t[old]) else "new DOES NOT WIN"
                ratios = [f"old/new {med[old] / med['new']:.2f}", f"new/copy {med['new'] / med['copy']:.2f}",
                          f"new reads at {n * esz / med['new'] * 1e-9:.2f} TB/s of one pass"]
                if "torch" in t:
                    ratios.append(f"torch/new {med['torch'] / med['new']:.2f}")
                print(f"{key:<5}{rows:>6} x {cols:<10}{label:<10}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
                      "  | " + "  ".join(ratios) + "  | " + verdict, file=out)
                out.flush()
                v.clear()
            del ws, sws, sk, si, cdst, ko, io
        del xall
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28, help="keys per shape: the four shapes scaled to about 2^logn keys")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--key", action="append", choices=list(DT), default=[])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--warmup", type=int, default=1, help="calls of each variant before the timed ones")
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", action="append", default=[], metavar="ROWSxCOLS", help="these shapes instead of the four")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kth_bench: no GPU (no CPU fallback)")
    shapes = [(1, 1 << a.logn) if r == 1 else (max(1, (r << a.logn) >> 28), c) for r, c in SHAPES]
    if a.shape:
        shapes = [tuple(int(v) for v in s.split("x")) for s in a.shape]
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.reps, out, a.key or list(DT), shapes, not a.no_torch, a.warmup)
