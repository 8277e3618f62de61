#!/usr/bin/env python3
"""Unique measurements on an MI355X.

2^logn32 int32 keys and 2^logn64 int64 keys of three inputs -- uniform over the full width (m ~ n),
% 1000 and % 2^20 -- and per input:
  new_k      labsort_unique_device, keys only
  new_c      ... with counts
  new_ic     ... with inverse and counts
  sort_k     the inner sort of new_k / new_c alone (labsort_sort_device; labsort_sort64_device without positions)
  sort_p     the inner sort of new_ic alone (labsort_sort_pairs_device on (key, iota); sort64 with positions)
  edge_ic    the run-edge passes alone: consecutive mode on the sorted keys, inverse and counts
  cons_k     consecutive mode on the sorted keys, keys only
  copy       labsort_copy of as many bytes as edge_ic moves (computed from n, m and the element sizes)
  composed   what a caller had before for values, inverse and counts: the pair sort on (key, iota), then
             torch !=, cumsum, index and scatter ops
  torch      torch.unique(sorted=True, return_inverse=True, return_counts=True)
Every variant of a case is timed in turn, repetition by repetition (device events around one call),
after --warmup calls each; median [min, max] ms.  new_ic is checked against torch.unique on the device.
Criterion per case (the one of DESIGN.md §3.16): the slowest repetition of new_ic below the fastest of
composed."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")

INPUTS = ["uniform", "mod1000", "mod2p20"]


def make(inp, n, dt):
    g = torch.Generator(device="cuda").manual_seed(0x0B1C)
    if inp == "uniform":
        if dt == torch.int32:
            return torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
        hi = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
        return (hi << 32) | torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
    mod = 1000 if inp == "mod1000" else 1 << 20
    return torch.randint(0, mod, (n,), dtype=torch.int64, device="cuda", generator=g).to(dt)


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


def run_case(inp, n, dt, reps, warmup, with_torch, out):
    key, esz = ("i32", 4) if dt == torch.int32 else ("i64", 8)
    x = make(inp, n, dt)
    words = lambda: torch.empty(n, dtype=torch.int32, device="cuda")  # noqa: E731
    uq, sk = torch.empty_like(x), torch.empty_like(x)
    counts, inverse, sp, num = words(), words(), words(), torch.zeros(1, dtype=torch.int32, device="cuda")
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    ws = torch.full((ls.unique_workspace_bytes(n, key, False, True),), 0xFF, dtype=torch.uint8, device="cuda")
    xs = torch.sort(x).values
    if key == "i32":
        sws = torch.empty(max(ls.pairs_workspace_bytes(n, "auto"), ls.workspace_bytes(n, "auto")), dtype=torch.uint8, device="cuda")
        sort_k = lambda: ls.sort_device(x, sk, n, key=key, algo="auto", workspace=sws)  # noqa: E731
        sort_p = lambda: ls.sort_pairs_device(x, iota, sk, sp, n, key=key, algo="auto", workspace=sws)  # noqa: E731
    else:
        sws = torch.empty(ls.sort64_workspace_bytes(1, n, True), dtype=torch.uint8, device="cuda")
        sort_k = lambda: ls.sort64_device(x, 1, n, sk, None, key=key, workspace=sws)  # noqa: E731
        sort_p = lambda: ls.sort64_device(x, 1, n, sk, sp, key=key, workspace=sws)  # noqa: E731
    res = {}

    def composed():
        sort_p()
        head = torch.ones(n, dtype=torch.bool, device="cuda")
        torch.ne(sk[1:], sk[:-1], out=head[1:])
        run = torch.cumsum(head, 0, dtype=torch.int32) - 1
        inv = torch.empty(n, dtype=torch.int32, device="cuda")
        inv[sp.long()] = run
        start = torch.nonzero(head).squeeze(1)  # (reads the number of runs back, as torch.unique does)
        res["c"] = sk[start], inv, torch.diff(start, append=start.new_tensor([n]))

    v = {"new_k": lambda: ls.unique_device(x, n, uq, num, key=key, workspace=ws),
         "new_c": lambda: ls.unique_device(x, n, uq, num, counts, key=key, workspace=ws),
         "new_ic": lambda: ls.unique_device(x, n, uq, num, counts, None, inverse, key=key, workspace=ws),
         "sort_k": sort_k, "sort_p": sort_p,
         "edge_ic": lambda: ls.unique_device(xs, n, uq, num, counts, None, inverse, key=key, consecutive=True, workspace=ws),
         "cons_k": lambda: ls.unique_device(xs, n, uq, num, key=key, consecutive=True, workspace=ws)}
    v["new_ic"]()
    m = int(num.item())
    # bytes of edge_ic: the count reads the keys, the write reads them again and stores the inverse; per
    # run a key, a start (stored, then read by the counts) and a count
    moved = n * (2 * esz + 4) + m * (esz + 12)
    cw = moved // 2 // 16 * 4  # words read, and as many written
    cb = torch.empty(8 * cw, dtype=torch.uint8, device="cuda")
    v["copy"] = lambda: ls.copy(cb, cb[4 * cw:], cw)
    v["composed"] = composed
    if with_torch:
        v["torch"] = lambda: res.__setitem__("t", torch.unique(x, sorted=True, return_inverse=True, return_counts=True))
    t = alternate(v, reps, warmup)
    v["new_ic"]()
    ls.unique_workspace_status(ws, n, key)
    tv, ti, tc = torch.unique(x, sorted=True, return_inverse=True, return_counts=True)
    assert int(num.item()) == tv.numel() == m
    assert torch.equal(uq[:m], tv) and torch.equal(inverse.long(), ti) and torch.equal(counts[:m].long(), tc), "new_ic differs"
    composed()
    torch.cuda.synchronize()
    assert torch.equal(res["c"][0], tv) and torch.equal(res["c"][1].long(), ti) and torch.equal(res["c"][2], tc), "composed differs"
    met = max(t["new_ic"]) < min(t["composed"])
    med = statistics.median
    notes = [f"edge_ic {moved / med(t['edge_ic']) * 1e-9:.2f} TB/s, copy {moved / med(t['copy']) * 1e-9:.2f} TB/s",
             f"new_ic/sort_p {med(t['new_ic']) / med(t['sort_p']):.2f}", f"new_k/sort_k {med(t['new_k']) / med(t['sort_k']):.2f}",
             f"composed/new_ic {med(t['composed']) / med(t['new_ic']):.2f}"]
    if with_torch:
        notes.append(f"torch/new_ic {med(t['torch']) / med(t['new_ic']):.2f}")
    notes.append("criterion " + ("met" if met else "NOT met") + f" (max new_ic {max(t['new_ic']):.3f}, min composed {min(t['composed']):.3f})")
    print(f"{key} {inp:<8} n = {n}  m = {m}", file=out)
    for name, ts in t.items():
        print(f"    {name:<9}{fmt(ts)}", file=out)
    print("    " + "; ".join(notes), file=out)
    out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn32", type=int, default=28)
    ap.add_argument("--logn64", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unique_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    print(f"# unique, {a.reps} alternating repetitions after {a.warmup} warm-up calls, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; chunk {ls.unique_chunk_keys()} keys", file=out)
    for dt, logn in ((torch.int32, a.logn32), (torch.int64, a.logn64)):
        for inp in a.inputs.split(","):
            run_case(inp, 1 << logn, dt, a.reps, a.warmup, not a.no_torch, out)
            torch.cuda.empty_cache()
