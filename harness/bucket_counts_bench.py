#!/usr/bin/env python3
"""Bucket-count and bincount measurements on an MI355X.

Cases (--cases picks by name), each with values as drawn (rand), sorted, and all equal (--dists):
  f32_255, f32_4095     2^logn float32 values on 255 / 4095 shared edges, one row of counts
  bf16_255, bf16_4095   the same in bfloat16
  rows_bf16             1767 rows of 151936 bfloat16 values on 255 shared edges, counts per row
  rows_f32              4096 rows of 4096 float32 values, 4096 edges per row
  long_i32              2^(logn-2) int32 values on 2^20 int32 edges (long path)
  bin_1000, bin_2p20    bincount of 2^logn int32 values in [0, nbins) at 1000 and at 2^20 bins
Variants:
  new     labsort_bucket_counts_device / labsort_bincount_device
  ls      the route of the parent commit: labsort_searchsorted_device into a rank array, then torch.bincount
          (counts per row: with the row's offset added to its ranks first)
  torch   torch.bucketize / torch.searchsorted (out_int32) into a rank array, then torch.bincount; for the
          bincount cases torch.bincount(minlength=nbins) alone
  copy    labsort_copy of the same input bytes (read once, written once)
  nocomb  with --ab-lib: the same entry of a library built with -DLABSORT_BC_COMBINE=0 (one atomic per
          value instead of one per run of equal neighbouring ranks of a thread)
Every variant of a case is timed in turn, repetition by repetition (device events around one call), after
--warmup calls each; median [min, max] ms.  The counts of new, ls, torch and nocomb are checked equal on
the device before the timing.  Criterion per case and old route (the one of DESIGN.md §3.16): the slowest
repetition of new below the fastest of the old route."""
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

CASES = ["f32_255", "f32_4095", "bf16_255", "bf16_4095", "rows_bf16", "rows_f32", "long_i32", "bin_1000", "bin_2p20"]
DISTS = ["rand", "sorted", "equal"]
KEY = {torch.int32: "i32", torch.float32: "f32", torch.bfloat16: "bf16"}


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


def shape_values(vals, dist):
    """rows x nv values as drawn, each row sorted, or every value the row's first."""
    if dist == "sorted":
        return vals.sort(dim=-1).values.contiguous()
    if dist == "equal":
        return vals[..., :1].expand(vals.shape).contiguous()
    return vals


def make(case, logn):
    """(edges or None, values rows x nv, nbins or None)"""
    g = torch.Generator(device="cuda").manual_seed(0x5EA7C4)
    n = 1 << logn
    randn = lambda *shape: torch.randn(shape, device="cuda", generator=g)  # noqa: E731
    if case.startswith(("f32_", "bf16_")):
        dt = torch.float32 if case.startswith("f32") else torch.bfloat16
        return randn(int(case.split("_")[1])).to(dt).sort().values, randn(1, n).to(dt), None
    if case == "rows_bf16":
        return randn(255).to(torch.bfloat16).sort().values, randn(1767, 151936).to(torch.bfloat16), None
    if case == "rows_f32":
        return randn(4096, 4096).sort(dim=-1).values.contiguous(), randn(4096, 4096), None
    if case == "long_i32":
        draw = lambda m: (torch.randint(0, 1 << 32, (m,), dtype=torch.int64, device="cuda", generator=g) - (1 << 31)).to(torch.int32)  # noqa: E731
        return draw(1 << 20).sort().values, draw(n >> 2).view(1, -1), None
    nbins = 1000 if case == "bin_1000" else 1 << 20
    return None, torch.randint(0, nbins, (1, n), dtype=torch.int32, device="cuda", generator=g), nbins


def ab_entry(path):
    lib = ctypes.CDLL(path)
    p, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.labsort_bucket_counts_device.argtypes = [p, sz, sz, p, sz, sz, i, i, p, p, sz, p]
    lib.labsort_bincount_device.argtypes = [p, sz, sz, sz, i, p, p]
    return lib


def run_case(case, dist, logn, reps, warmup, out, ab):
    edges, vals, nbins = make(case, logn)
    vals = shape_values(vals, dist)
    rows, nv = vals.shape
    key = KEY[vals.dtype]
    nb = (nbins if edges is None else edges.shape[-1]) + 1
    new = torch.full((rows, nb), -1, dtype=torch.int32, device="cuda")
    copy_out = torch.empty_like(vals)
    v, old = {}, {}
    if edges is None:
        v["new"] = lambda: ls.bincount_device(vals, rows, nv, nbins, new, key=key)
        old["torch"] = lambda: torch.bincount(vals.view(-1), minlength=nbins)
        path = "LDS counters" if nbins <= ls.bincount_row_bins() else "global atomics"
        if ab is not None:
            abo = torch.full_like(new, -1)
            v["nocomb"] = lambda: ab.labsort_bincount_device(vals.data_ptr(), rows, nv, nbins, ls.KEY[key], abo.data_ptr(), None)
    else:
        edge_rows, nedges = edges.shape if edges.dim() == 2 else (1, edges.shape[0])
        need = ls.bucket_counts_workspace_bytes(edge_rows, nedges, key)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda") if need else None
        path = "long path" if need else "LDS path"
        v["new"] = lambda: ls.bucket_counts_device(edges, edge_rows, nedges, vals, rows, nv, new, key=key, workspace=ws)
        if ab is not None:
            abo = torch.full_like(new, -1)
            v["nocomb"] = lambda: ab.labsort_bucket_counts_device(edges.data_ptr(), edge_rows, nedges, vals.data_ptr(), rows, nv, 0, ls.KEY[key],
                                                                  abo.data_ptr(), ws.data_ptr() if need else None, need, None)
        ranks = torch.empty((rows, nv), dtype=torch.int32, device="cuda")
        offs = (torch.arange(rows, device="cuda", dtype=torch.int32) * nb).view(-1, 1)
        sneed = ls.searchsorted_workspace_bytes(edge_rows, nedges, key)
        sws = torch.full((sneed,), 0xFF, dtype=torch.uint8, device="cuda") if sneed else None
        # with one shared sequence searchsorted takes all the values as one row
        srows, snv = (rows, nv) if edge_rows != 1 else (1, rows * nv)

        def count(r):
            return torch.bincount((r + offs).view(-1) if rows > 1 else r.view(-1), minlength=rows * nb)

        def ls_route():
            ls.searchsorted_device(edges, edge_rows, nedges, vals, srows, snv, ranks, key=key, workspace=sws)
            return count(ranks)

        def torch_route():
            if edge_rows == 1:
                torch.bucketize(vals, edges, out_int32=True, out=ranks)
            else:
                torch.searchsorted(edges, vals, out_int32=True, out=ranks)
            return count(ranks)

        old["ls"], old["torch"] = ls_route, torch_route
    nwords = vals.numel() * vals.element_size() // 4
    v["copy"] = lambda: ls.copy(vals, copy_out, nwords)
    v["new"]()
    torch.cuda.synchronize()
    assert bool((new.sum(dim=1) == nv).all()), f"{case} {dist}: a row of new does not sum to nv"
    refused = {}
    for name, fn in old.items():
        try:
            got = fn()
            torch.cuda.synchronize()
        except (RuntimeError, TypeError, NotImplementedError) as e:  # a dtype torch does not take: written down, not timed
            refused[name] = str(e).splitlines()[0]
            continue
        want = new.view(-1) if edges is not None else new.view(-1)[:nbins]
        assert torch.equal(got.int(), want), f"{case} {dist}: new differs from {name}"
        v[name] = fn
    if "nocomb" in v:
        v["nocomb"]()
        torch.cuda.synchronize()
        assert torch.equal(abo, new), f"{case} {dist}: nocomb differs from new"
    t = alternate(v, reps, warmup)
    med = statistics.median
    print(f"{case} {dist}: {key} values {rows} x {nv}, " + (f"{nbins} bins" if edges is None else f"edges {edge_rows} x {nedges}") +
          f", {path}", file=out)
    for name, ts in t.items():
        print(f"    {name:<7}{fmt(ts)}", file=out)
    notes = [f"new {vals.numel() * vals.element_size() / med(t['new']) * 1e-9:.3f} TB/s of values read", f"new/copy {med(t['new']) / med(t['copy']):.2f}"]
    for route in old:
        if route in refused:
            notes.append(f"{route} refuses: {refused[route]}")
        else:
            met = max(t["new"]) < min(t[route])
            notes.append(f"{route}/new {med(t[route]) / med(t['new']):.2f}, criterion vs {route} " + ("met" if met else "NOT met") +
                         f" (max new {max(t['new']):.3f}, min {route} {min(t[route]):.3f})")
    if "nocomb" in t:
        notes.append(f"nocomb/new {med(t['nocomb']) / med(t['new']):.2f} (max new {max(t['new']):.3f}, min nocomb {min(t['nocomb']):.3f})")
    print("    " + "; ".join(notes), file=out)
    out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--dists", default=",".join(DISTS))
    ap.add_argument("--ab-lib", default="", help="a liblabsort.so built with -DLABSORT_BC_COMBINE=0, timed as nocomb")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bucket_counts_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    print(f"# bucket counts, {a.reps} alternating repetitions after {a.warmup} warm-up calls, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; chunk {ls.searchsorted_chunk_values()} values, LDS path up to "
          f"{ls.bucket_counts_row_edges('f32')} 4-byte edges, bincount LDS counters up to {ls.bincount_row_bins()} bins", file=out)
    ab = ab_entry(a.ab_lib) if a.ab_lib else None
    for case in a.cases.split(","):
        for dist in a.dists.split(","):
            run_case(case, dist, a.logn, a.reps, a.warmup, out, ab)
            torch.cuda.empty_cache()
