#!/usr/bin/env python3
"""64-bit key sort measurements on an MI355X (output kept in profiles/sort64.txt).

2^logn keys as rows x cols -- one row of 2^logn keys, rows of 131072 and rows of 4096 keys -- of four
inputs: u64 uniform over the full width, i64 uniform in [0, 2^32), i64 of small magnitude and mixed
sign (-1000 .. 1000), f64 standard normals; sorted ascending with positions:
  new       labsort_sort64_device with positions; `passes` is the plan the device made
  new_k     the same without positions
  torch     torch.sort(x, dim=-1, stable=True) on the same tensor (u64: on its int64 view, the same work)
  composed  one row of integer keys only: what a caller could do before -- the words split,
            labsort_sort_pairs_device on the low words with an iota, a gather of the high words by the
            positions, labsort_sort_pairs_device on those, a final gather of the keys
  copy      labsort_copy of the input's bytes (one read and one write of the keys)
Every variant of a case is timed in turn, repetition by repetition (device events around one call),
after --warmup calls each; median [min, max] ms over the repetitions.  The result of `new` is checked on
the device: the keys are the input gathered by the positions, their images do not descend, and
positions ascend within equal images.
--one CASE (with --shape): only `new` of one input on one shape, --reps times -- what a kernel trace
is taken of (harness/exp/ktrace.py prints the sequence)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

SHAPES = [(1, 1 << 27), (1024, 131072), (32768, 4096)]
INPUTS = ["u64_full", "i64_lt2p32", "i64_small_mixed", "f64_normal"]
KEY = {"u64_full": "u64", "i64_lt2p32": "i64", "i64_small_mixed": "i64", "f64_normal": "f64"}
SIGN = -(1 << 63)


def make(inp, n):
    g = torch.Generator(device="cuda").manual_seed(0x64BE)
    if inp == "u64_full":
        hi = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
        return (hi << 32) | torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
    if inp == "i64_lt2p32":
        return torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
    if inp == "i64_small_mixed":
        return torch.randint(-1000, 1001, (n,), dtype=torch.int64, device="cuda", generator=g)
    return torch.randn(n, dtype=torch.float64, device="cuda", generator=g)


def image(x, key):
    """The order image as int64 whose signed order is the image's unsigned one (NaN-free inputs)."""
    w = x.view(torch.int64)
    if key == "i64":
        return w
    if key == "u64":
        return w ^ SIGN
    return torch.where(w < 0, ~w ^ SIGN, w)  # f64: (~w) ^ SIGN below zero, (w | SIGN) ^ SIGN = w otherwise


def verify(x, ko, io, rows, cols, key):
    xi, ki = x.view(torch.int64).view(rows, cols), ko.view(torch.int64).view(rows, cols)
    idx = io.view(rows, cols).long()
    assert torch.equal(torch.gather(xi, 1, idx), ki), "keys are not the input gathered by the positions"
    u = image(ki, key)
    assert bool((u[:, 1:] >= u[:, :-1]).all()), "images descend"
    tie = u[:, 1:] == u[:, :-1]
    assert bool((idx[:, 1:] > idx[:, :-1])[tie].all()), "equal keys out of position order"
    assert bool((idx.sort(dim=1).values == torch.arange(cols, device="cuda")).all()), "positions are no permutation"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, warmup=1):
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


def composed_route(x, n, key):
    """The one-row route through two key/value sorts of 32-bit words; returns (fn, keys out, positions)."""
    pw = torch.full((ls.pairs_workspace_bytes(n, "radix"),), 0xFF, dtype=torch.uint8, device="cuda")
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    lo_s, hi_s, p1, p2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))
    out = {}

    def fn():
        w = x.view(torch.int32).view(n, 2)
        lo, hi = w[:, 0].contiguous(), w[:, 1].contiguous()
        ls.sort_pairs_device(lo, iota, lo_s, p1, n, key="u32", algo="radix", workspace=pw)
        hg = torch.index_select(hi, 0, p1)
        ls.sort_pairs_device(hg, p1, hi_s, p2, n, key="u32" if key == "u64" else "i32", algo="radix", workspace=pw)
        out["k"] = torch.index_select(x, 0, p2)
    return fn, out, p2


def run_case(inp, rows, cols, reps, warmup, with_torch, out):
    n, key = rows * cols, KEY[inp]
    x = make(inp, n)
    ko, ko2 = torch.empty_like(x), torch.empty_like(x)
    io = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.full((ls.sort64_workspace_bytes(rows, cols, True),), 0xFF, dtype=torch.uint8, device="cuda")
    v = {"new": lambda: ls.sort64_device(x, rows, cols, ko, io, key=key, workspace=ws),
         "new_k": lambda: ls.sort64_device(x, rows, cols, ko2, None, key=key, workspace=ws)}
    if with_torch:
        xt = x.view(torch.int64) if key == "u64" else x
        v["torch"] = lambda: torch.sort(xt.view(rows, cols), dim=-1, stable=True)
    comp = None
    if rows == 1 and key != "f64":
        fn, comp, p2 = composed_route(x, n, key)
        v["composed"] = fn
    v["copy"] = lambda: ls.copy(x, ko2, 2 * n)
    t = alternate(v, reps, warmup)
    v["new"]()
    ls.sort64_workspace_status(ws)
    passes = ls.sort64_passes(ws)
    verify(x, ko, io, rows, cols, key)
    v["new_k"]()
    torch.cuda.synchronize()
    assert torch.equal(ko.view(torch.int64), ko2.view(torch.int64)), "keys without positions differ"
    if comp is not None:
        v["composed"]()
        torch.cuda.synchronize()
        assert torch.equal(comp["k"], ko) and torch.equal(p2, io), "the composed route's result differs"
    m = bin(passes).count("1") if cols > ls.sort64_chunk_keys() else None
    ratios = [f"new/copy {med(t['new']) / med(t['copy']):.2f}", f"copy {16 * n / med(t['copy']) * 1e-9:.2f} TB/s"]
    if m:
        ratios.append(f"new {32 * m * n / med(t['new']) * 1e-9:.2f} TB/s at 32 B/key/pass")
    if with_torch:
        ratios.append(f"torch/new {med(t['torch']) / med(t['new']):.2f}")
    if comp is not None:
        ratios.append(f"composed/new {med(t['composed']) / med(t['new']):.2f}")
    plan = f"passes {passes:#04x} (m = {m})" if m is not None else "one workgroup per row"
    print(f"{inp:<16}{rows:>6} x {cols:<10}{plan:<24}" + "  ".join(f"{name} {fmt(ts)}" for name, ts in t.items()) +
          "  | " + "  ".join(ratios), file=out)
    out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=27, help="keys per shape: the three shapes scaled to 2^logn keys")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1, help="calls of each variant before the timed ones")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--shape", type=int, default=-1, help="only this one of the three shapes (0, 1, 2)")
    ap.add_argument("--one", default="", metavar="INPUT", help="only `new` of this input, --reps times (for a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sort64_bench: no GPU (no CPU fallback)")
    shapes = [(1, 1 << a.logn) if r == 1 else (max(1, (r << a.logn) >> 27), c) for r, c in SHAPES]
    if a.shape >= 0:
        shapes = [shapes[a.shape]]
    out = open(a.out, "a") if a.out else sys.stdout
    if a.one:
        rows, cols = shapes[0]
        x = make(a.one, rows * cols)
        ko, io = torch.empty_like(x), torch.empty(rows * cols, dtype=torch.int32, device="cuda")
        ws = torch.full((ls.sort64_workspace_bytes(rows, cols, True),), 0xFF, dtype=torch.uint8, device="cuda")
        for _ in range(a.reps):
            ls.sort64_device(x, rows, cols, ko, io, key=KEY[a.one], workspace=ws)
        print(f"{a.one} {rows} x {cols}: passes {ls.sort64_passes(ws):#04x}", file=out)
        sys.exit(0)
    print(f"# 64-bit key sort, ascending, {a.reps} alternating repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; chunk {ls.sort64_chunk_keys()} keys", file=out)
    for rows, cols in shapes:
        for inp in a.inputs.split(","):
            run_case(inp, rows, cols, a.reps, a.warmup, not a.no_torch, out)
