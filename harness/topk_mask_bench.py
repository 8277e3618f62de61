#!/usr/bin/env python3
"""Top-k filtering measurements on an MI355X (output kept in profiles/topk_mask.txt).

Standard normals as rows x cols -- harness/kth_bench.py's shapes and 5341 x 50257 -- as float32, rounded
to bfloat16, or in fixed point as int32; every row with all but its k largest keys set to -inf (int32:
the smallest integer), keys output only, out of place and in place, for k = 1, 50, 1024 and a random k
per row:
  new               labsort_topk_mask_device (a host k, or d_k for the k per row)
  old:kth+torch     labsort_kth_device with positions, then torch: gt, eq, an arange compare, and, or and
                    where, every output preallocated (the plain comparisons are the library's order on
                    this input: no NaN, no zero of either sign among the keys at the threshold)
  old:topk+scatter  where k is one value and k <= cols / 4: labsort_topk_device(k), the positions widened
                    to int64, a fill and a scatter_ of the survivors
  kth               the select alone: the labsort_kth_device call of old:kth+torch (new - kth is what the
                    apply pass costs)
  copy              labsort_copy of the matrix's bytes (one read and one write)
In place, the matrix is restored from a copy before every call, outside the timed region.  Every variant
of a case is timed in turn, repetition by repetition (device events around one call), after --warmup
calls each; ms: median [min, max] over the repetitions.  `wins`: new's maximum lies below the minimum of
the fastest old route that applies.  Before the timing new's output is compared with both old routes'."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ls = importlib.import_module("radix-sort-merge-sort-cuda---lab-y-practicos-gpgpu-2023_amd")
import kth_bench as KB  # noqa: E402  (the shapes, the keys and the timing loop's parts)

DT = KB.DT
SHAPES = KB.SHAPES + [(5341, 50257)]


def alternate(variants, reps, warmup, before):
    """kth_bench.alternate with before[name]() run ahead of every call, untimed."""
    def once(name, fn, keep):
        if name in before:
            before[name]()
        ms = KB.timed(fn)
        if keep is not None:
            keep.append(ms)
    for _ in range(warmup):
        for name, fn in variants.items():
            once(name, fn, None)
    torch.cuda.synchronize()
    t = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            once(name, fn, t[name])
    return t


def main(reps, out, keys, shapes, warmup):
    print(f"# top-k filter (largest, keys output only), standard-normal keys, {reps} alternating repetitions after {warmup} "
          f"warm-ups, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; one launch up to {ls.kth_row_keys()} keys per row; "
          f"library {os.path.basename(ls.LIB_PATH)}", file=out)
    for key in keys:
        xall = KB.make_keys(key, max(r * c for r, c in shapes))
        esz = xall.element_size()
        fillv = torch.iinfo(torch.int32).min if key == "i32" else float("-inf")
        fill_bits = ls._fill_bits(xall.dtype, fillv)
        fillt = torch.tensor(fillv, dtype=xall.dtype, device="cuda")
        for rows, cols in shapes:
            n = rows * cols
            x = xall[:n].view(rows, cols)
            y = torch.empty_like(x)  # the matrix that is filtered in place
            res = torch.empty_like(x)
            oldres = torch.empty_like(x)
            ws = torch.full((ls.topk_mask_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
            kws = torch.full((ls.kth_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
            kT = torch.empty(rows, dtype=xall.dtype, device="cuda")
            kP = torch.empty(rows, dtype=torch.int32, device="cuda")
            m1, m2, m3 = (torch.empty((rows, cols), dtype=torch.bool, device="cuda") for _ in range(3))
            ar = torch.arange(cols, dtype=torch.int32, device="cuda").view(1, cols)
            cdst = torch.empty(n * esz // 4, dtype=torch.int32, device="cuda")
            g = torch.Generator(device="cuda").manual_seed(0x4B7EED + cols)
            kper = torch.randint(1, cols + 1, (rows,), generator=g, device="cuda", dtype=torch.int32)

            def kth(src, k):
                ls.kth_device(src, rows, cols, k, kT, kP, largest=True, key=key, workspace=kws)

            def kth_torch(src, dst, k):
                kth(src, k)
                t = kT.view(rows, 1)
                torch.gt(src, t, out=m1)
                torch.eq(src, t, out=m2)
                torch.le(ar, kP.view(rows, 1), out=m3)
                m2.logical_and_(m3)
                m1.logical_or_(m2)
                torch.where(m1, src, fillt, out=dst)

            for label, k in (("k=1", 1), ("k=50", 50), ("k=1024", 1024), ("k per row", kper)):
                per_row = not isinstance(k, int)
                if not per_row and k > cols:
                    continue
                topk_ok = not per_row and k * 4 <= cols
                if topk_ok:
                    tk = torch.empty((rows, k), dtype=xall.dtype, device="cuda")
                    ti = torch.empty((rows, k), dtype=torch.int32, device="cuda")
                    ti64 = torch.empty((rows, k), dtype=torch.int64, device="cuda")
                    tws = torch.full((ls.topk_workspace_bytes(rows, cols, k),), 0xFF, dtype=torch.uint8, device="cuda")

                    def topk_scatter(src, dst, k=k, tk=tk, ti=ti, ti64=ti64, tws=tws):
                        ls.topk_device(src, rows, cols, k, tk, ti, largest=True, key=key, workspace=tws)
                        ti64.copy_(ti)
                        dst.fill_(fillv)
                        dst.scatter_(1, ti64, tk)
                for place in ("out", "in"):
                    src, dst = (x, res) if place == "out" else (y, y)
                    odst = oldres if place == "out" else y
                    restore = (lambda: y.copy_(x)) if place == "in" else None
                    v = {"new": lambda k=k: ls.topk_mask_device(src, rows, cols, k, d_keys_out=dst, largest=True, fill_bits=fill_bits,
                                                                key=key, workspace=ws)}
                    v["old:kth+torch"] = lambda k=k: kth_torch(src, odst, k)
                    if topk_ok:
                        v["old:topk+scatter"] = lambda: topk_scatter(src, odst)
                    v["kth"] = lambda k=k: kth(x, k)
                    v["copy"] = lambda: ls.copy(x, cdst, n * esz // 4)
                    olds = [name for name in v if name.startswith("old:")]
                    before = {name: restore for name in ["new"] + olds} if restore else {}
                    # new's output is both old routes', bit for bit
                    if restore:
                        restore()
                    v["new"]()
                    ls.topk_mask_workspace_status(ws)
                    got = dst.clone()
                    for name in olds:
                        if restore:
                            restore()
                        v[name]()
                        torch.cuda.synchronize()
                        assert torch.equal(KB.bits(got), KB.bits(odst)), (key, rows, cols, label, place, name)
                    kept = (got != fillt).sum(dim=1)
                    assert torch.equal(kept, kper.long() if per_row else torch.full_like(kept, k)), (key, rows, cols, label, place)
                    t = alternate(v, reps, warmup, before)
                    med = {name: statistics.median(ts) for name, ts in t.items()}
                    best_old = min(olds, key=lambda name: min(t[name]))
                    verdict = "new wins" if max(t["new"]) < min(t[best_old]) else "new DOES NOT WIN"
                    apply_ms = med["new"] - med["kth"]
                    ratios = [f"best old {best_old} / new {med[best_old] / med['new']:.2f}", f"new/copy {med['new'] / med['copy']:.2f}",
                              f"new-kth {apply_ms:.3f} ms = {apply_ms / med['copy']:.2f} copy = {2 * n * esz / max(apply_ms, 1e-6) * 1e-9:.2f} TB/s of one read and one write"]
                    print(f"{key:<5}{rows:>6} x {cols:<10}{label:<10}{place:<4}" + "  ".join(f"{name} {KB.fmt(ts)}" for name, ts in t.items()) +
                          "  | " + "  ".join(ratios) + "  | " + verdict, file=out)
                    out.flush()
                    v.clear()
            del ws, kws, y, res, oldres, m1, m2, m3, ar, cdst
        del xall
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28, help="keys per shape: kth_bench's four shapes scaled to about 2^logn keys")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--key", action="append", choices=list(DT), default=[])
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", action="append", default=[], metavar="ROWSxCOLS", help="these shapes instead of the five")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_mask_bench: no GPU (no CPU fallback)")
    shapes = [(1, 1 << a.logn) if r == 1 else (max(1, (r << a.logn) >> 28), c) if (r, c) in KB.SHAPES else (r, c) for r, c in SHAPES]
    if a.shape:
        shapes = [tuple(int(v) for v in s.split("x")) for s in a.shape]
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.reps, out, a.key or list(DT), shapes, a.warmup)
