#!/usr/bin/env python3
"""Top-p filtering measurements on an MI355X (output kept in profiles/top_p.txt).

Rows of softmax(standard-normal logits / temperature) at two temperatures as rows x cols, float32 or
rounded to bfloat16; every row reduced to its top-p set with 0 elsewhere, keys output only, out of place
and in place, for p = 0.5, 0.9, 0.99 and a random p per row:
  new          labsort_top_p_device (a host p, or d_p for the p per row), the counts written too
  old:torch    torch.sort(descending=True, stable=True), a cumsum, a compare against p times the row's
               sum and a scatter back, every output preallocated
  old:labsort  ls.sort(x, descending=True), a cumsum and a compare for each row's count, then
               labsort_topk_mask_device with that d_k
  topk_mask    labsort_topk_mask_device given new's counts beforehand: what the count select costs, the
               floor the mass select is read against
  copy         labsort_copy of the matrix's bytes (one read and one write)
In place, the matrix is restored from a copy before every call, outside the timed region.  Every variant
of a case is timed in turn, repetition by repetition (device events around one call), after --warmup
calls each; ms: median [min, max] over the repetitions.  `wins`: new's maximum lies below the minimum of
the fastest old route.  The old routes sum floats, so before the timing the counts are not compared for
equality: with m(n) the float64 mass of a row's first n sorted entries and M = m(cols), new's k of every
row must lie in the band m(k) >= p M - e, m(k - 1) < p M + e, e = 2^-32 M + cols 2^-40 (asserted), and
for each old route the rows whose k equals new's and the rows whose k lies in the band are counted."""
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
import kth_bench as KB  # noqa: E402  (the timing loop's parts)
from topk_mask_bench import alternate  # noqa: E402

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [(1767, 151936), (5341, 50257), (65536, 4096), (4096, 65536)]
TEMPERATURES = (1.0, 0.7)


def make_probs(key, rows, cols, temperature):
    z = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    z.normal_(generator=torch.Generator(device="cuda").manual_seed(0x70BEED + cols))
    return torch.softmax(z / temperature, dim=1).to(DT[key])


def main(reps, out, keys, shapes, warmup):
    print(f"# top-p filter (keys output and counts, fill 0), softmax of standard-normal logits, {reps} alternating repetitions "
          f"after {warmup} warm-ups, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; one launch up to {ls.kth_row_keys()} keys per row; "
          f"library {os.path.basename(ls.LIB_PATH)}", file=out)
    for key in keys:
        for rows, cols in shapes:
            n = rows * cols
            for temperature in TEMPERATURES:
                x = make_probs(key, rows, cols, temperature)
                esz = x.element_size()
                y = torch.empty_like(x)  # the matrix that is filtered in place
                res, oldres = torch.empty_like(x), torch.empty_like(x)
                ws = torch.full((ls.top_p_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
                mws = torch.full((ls.topk_mask_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device="cuda")
                kept = torch.empty(rows, dtype=torch.int32, device="cuda")
                kold = torch.empty(rows, dtype=torch.int32, device="cuda")
                sv, si = torch.empty_like(x), torch.empty((rows, cols), dtype=torch.int64, device="cuda")
                cum, keep = torch.empty((rows, cols), dtype=torch.float32, device="cuda"), torch.empty((rows, cols), dtype=torch.bool, device="cuda")
                cdst = torch.empty(n * esz // 4, dtype=torch.int32, device="cuda")
                zero = torch.zeros((), dtype=x.dtype, device="cuda")
                g = torch.Generator(device="cuda").manual_seed(0x70BEEE + cols)
                pper = torch.rand((rows,), generator=g, device="cuda", dtype=torch.float32).clamp_(min=2.0 ** -20)
                # float64 masses of the sorted rows, for the band
                m64 = torch.sort(x.double(), dim=1, descending=True).values.cumsum(dim=1)
                m64 = torch.cat([torch.zeros((rows, 1), dtype=torch.float64, device="cuda"), m64], dim=1)
                M = m64[:, cols]
                eband = 2.0 ** -32 * M + cols * 2.0 ** -40

                def in_band(k, pt):
                    k = k.long().view(rows, 1)
                    return (m64.gather(1, k).view(-1) >= pt * M - eband) & (m64.gather(1, k - 1).view(-1) < pt * M + eband)

                def kept_of_sorted(vals, pt):
                    """vals sorted descending -> keep (bool): the prefix whose exclusive float32 sum lies below p times the sum."""
                    torch.cumsum(vals, dim=1, dtype=torch.float32, out=cum)
                    lim = cum[:, -1:] * pt.view(rows, 1)
                    torch.lt(cum - vals, lim, out=keep)

                def old_torch(src, dst, pt):
                    torch.sort(src, dim=1, descending=True, stable=True, out=(sv, si))
                    kept_of_sorted(sv, pt)
                    dst.fill_(0)
                    dst.scatter_(1, si, torch.where(keep, sv, zero))

                def old_labsort(src, dst, pt):
                    vals, _ = ls.sort(src, descending=True)
                    kept_of_sorted(vals, pt)
                    torch.sum(keep, dim=1, dtype=torch.int32, out=kold)
                    ls.topk_mask_device(src, rows, cols, kold, d_keys_out=dst, largest=True, fill_bits=0, key=key, workspace=mws)

                for label, p in (("p=0.5", 0.5), ("p=0.9", 0.9), ("p=0.99", 0.99), ("p per row", pper)):
                    pt = p if isinstance(p, torch.Tensor) else torch.full((rows,), p, dtype=torch.float32, device="cuda")
                    pt64 = pt.double()
                    for place in ("out", "in"):
                        src, dst = (x, res) if place == "out" else (y, y)
                        odst = oldres if place == "out" else y
                        restore = (lambda: y.copy_(x)) if place == "in" else None
                        v = {"new": lambda p=p: ls.top_p_device(src, rows, cols, p, d_keys_out=dst, d_kept_out=kept, fill_bits=0,
                                                                key=key, workspace=ws),
                             "old:torch": lambda: old_torch(src, odst, pt), "old:labsort": lambda: old_labsort(src, odst, pt)}
                        olds = [name for name in v if name.startswith("old:")]
                        before = {name: restore for name in ["new", "topk_mask"] + olds} if restore else {}
                        if restore:
                            restore()
                        v["new"]()
                        ls.top_p_workspace_status(ws)
                        knew = kept.clone()
                        assert bool(in_band(knew, pt64).all()), (key, rows, cols, temperature, label, place, "new outside the band")
                        assert torch.equal((dst != 0).sum(dim=1).int(), knew), (key, rows, cols, label, place)
                        notes = []
                        for name in olds:
                            if restore:
                                restore()
                            v[name]()
                            torch.cuda.synchronize()
                            ko = (odst != 0).sum(dim=1).int()
                            notes.append(f"{name} k == new's in {int((ko == knew).sum())}, in the band in {int(in_band(ko.clamp(min=1), pt64).sum())} of {rows} rows")
                        v["topk_mask"] = lambda: ls.topk_mask_device(src, rows, cols, knew, d_keys_out=dst, largest=True, fill_bits=0,
                                                                     key=key, workspace=mws)
                        v["copy"] = lambda: ls.copy(x, cdst, n * esz // 4)
                        t = alternate(v, reps, warmup, before)
                        med = {name: statistics.median(ts) for name, ts in t.items()}
                        best_old = min(olds, key=lambda name: min(t[name]))
                        verdict = "new wins" if max(t["new"]) < min(t[best_old]) else "new DOES NOT WIN"
                        ratios = [f"best old {best_old} / new {med[best_old] / med['new']:.2f}", f"new/topk_mask {med['new'] / med['topk_mask']:.2f}",
                                  f"new/copy {med['new'] / med['copy']:.2f}", f"mean k {float(knew.float().mean()):.0f}"]
                        print(f"{key:<5}{rows:>6} x {cols:<8}T={temperature:<4}{label:<10}{place:<4}" + "  ".join(f"{name} {KB.fmt(ts)}" for name, ts in t.items()) +
                              "  | " + "  ".join(ratios) + "  | " + verdict + "  | " + "; ".join(notes), file=out)
                        out.flush()
                        v.clear()
                del x, y, res, oldres, ws, mws, sv, si, cum, keep, cdst, m64
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--key", action="append", choices=list(DT), default=[])
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", action="append", default=[], metavar="ROWSxCOLS", help="these shapes instead of the four")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("top_p_bench: no GPU (no CPU fallback)")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shape] if a.shape else SHAPES
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.reps, out, a.key or list(DT), shapes, a.warmup)
