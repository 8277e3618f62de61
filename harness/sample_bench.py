#!/usr/bin/env python3
"""Categorical sampling measurements on an MI355X (output kept in profiles/sample.txt).

Rows of softmax(standard-normal logits / temperature) at two temperatures as rows x cols, float32 or
rounded to bfloat16; ndraw positions drawn from every row:
  new              labsort_sample_device on preallocated random words
  old:multinomial  torch.multinomial(x, ndraw, replacement=True) on the tensor as it is (widened to float32
                   inside the timed region only where torch refuses the dtype; the line then says so)
  old:cumsum       a float32 torch.cumsum into a preallocated buffer, the target u x last column, and
                   torch.searchsorted(right=True) with a sequence per row
  old:race         argmax(x / Exp(1)), the exponentials drawn inside the timed region as samplers do, once
                   per draw
  copy             labsort_copy of the matrix's bytes (one read and one write)
Every variant of a case is timed in turn, repetition by repetition (device events around one call), after
--warmup calls each; ms: median [min, max] over the repetitions.  `wins`: new's maximum lies below the
minimum of the fastest old route.  Before the timing new is checked on a sample of rows against a float64
cumulative sum c: with W = c[cols - 1], u = U / 2^32 and j the position drawn, c[j - 1] - e <= u W <
c[j] + e, e = 2^-32 W + cols 2^-40 (asserted); and the draws in which old:cumsum, given the same u,
finds the same position are counted."""
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
SHAPES = [(1767, 151936, 1), (5341, 50257, 1), (65536, 4096, 1), (4096, 65536, 1), (65536, 4096, 8)]
TEMPERATURES = (1.0, 0.7)
CHECK_ROWS = 64


def make_probs(key, rows, cols, temperature):
    z = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    z.normal_(generator=torch.Generator(device="cuda").manual_seed(0x5A3BED + cols))
    return torch.softmax(z / temperature, dim=1).to(DT[key])


def main(reps, out, keys, shapes, warmup):
    print(f"# categorical sampling, softmax of standard-normal logits, {reps} alternating repetitions after {warmup} warm-ups, "
          f"ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}; one launch up to {ls.kth_row_keys()} keys per row; "
          f"library {os.path.basename(ls.LIB_PATH)}", file=out)
    for key in keys:
        for rows, cols, ndraw in shapes:
            n = rows * cols
            for temperature in TEMPERATURES:
                x = make_probs(key, rows, cols, temperature)
                esz = x.element_size()
                g = torch.Generator(device="cuda").manual_seed(0x5A3BEE + cols)
                words = (torch.randint(0, 1 << 16, (rows, ndraw), dtype=torch.int32, device="cuda", generator=g) << 16) | \
                    torch.randint(0, 1 << 16, (rows, ndraw), dtype=torch.int32, device="cuda", generator=g)
                u64 = (words.long() & 0xFFFFFFFF).double() / 4294967296.0
                uf = u64.float().clamp_(max=1.0 - 2.0 ** -24)  # what the float routes are given
                idx = torch.empty((rows, ndraw), dtype=torch.int32, device="cuda")
                ws = torch.full((ls.sample_workspace_bytes(rows, cols, ndraw),), 0xFF, dtype=torch.uint8, device="cuda")
                cum = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
                tgt = torch.empty((rows, ndraw), dtype=torch.float32, device="cuda")
                cidx = torch.empty((rows, ndraw), dtype=torch.int64, device="cuda")
                expo, quot = torch.empty_like(x), torch.empty_like(x)
                ridx = torch.empty((ndraw, rows), dtype=torch.int64, device="cuda")
                cdst = torch.empty(n * esz // 4, dtype=torch.int32, device="cuda")

                def new():
                    ls.sample_device(x, rows, cols, words, ndraw, idx, key=key, workspace=ws)

                def old_cumsum():
                    torch.cumsum(x, dim=1, dtype=torch.float32, out=cum)
                    torch.mul(uf, cum[:, -1:], out=tgt)
                    torch.searchsorted(cum, tgt, right=True, out=cidx)

                def old_race():
                    for d in range(ndraw):
                        expo.exponential_()
                        torch.div(x, expo, out=quot)
                        torch.argmax(quot, dim=1, out=ridx[d])

                widened = ""
                try:
                    torch.multinomial(x, ndraw, replacement=True)

                    def old_multinomial():
                        torch.multinomial(x, ndraw, replacement=True)
                except RuntimeError:
                    widened = " (old:multinomial on x.float(): torch refuses the dtype)"

                    def old_multinomial():
                        torch.multinomial(x.float(), ndraw, replacement=True)
                # the sanity check: new against a float64 cumulative sum on a sample of rows
                new()
                ls.sample_workspace_status(ws)
                pick = torch.linspace(0, rows - 1, min(rows, CHECK_ROWS), device="cuda").long()
                c64 = x[pick].double().cumsum(dim=1)
                c64 = torch.cat([torch.zeros((pick.numel(), 1), dtype=torch.float64, device="cuda"), c64], dim=1)
                W = c64[:, cols:cols + 1]
                e = 2.0 ** -32 * W + cols * 2.0 ** -40
                j = idx[pick].long()
                assert bool(((j >= 0) & (j < cols)).all()), (key, rows, cols, "a position outside the row")
                uw = u64[pick] * W
                assert bool(((c64.gather(1, j) - e <= uw) & (uw < c64.gather(1, j + 1) + e)).all()), (key, rows, cols, temperature, "new outside the float64 range")
                old_cumsum()
                torch.cuda.synchronize()
                same = int((cidx.clamp(max=cols - 1) == idx.long()).sum())
                v = {"new": new, "old:multinomial": old_multinomial, "old:cumsum": old_cumsum, "old:race": old_race,
                     "copy": lambda: ls.copy(x, cdst, n * esz // 4)}
                olds = [name for name in v if name.startswith("old:")]
                t = alternate(v, reps, warmup, {})
                med = {name: statistics.median(ts) for name, ts in t.items()}
                best_old = min(olds, key=lambda name: min(t[name]))
                verdict = "new wins" if max(t["new"]) < min(t[best_old]) else "new DOES NOT WIN"
                print(f"{key:<5}{rows:>6} x {cols:<8}ndraw={ndraw:<3}T={temperature:<4}" + "  ".join(f"{name} {KB.fmt(ts)}" for name, ts in t.items()) +
                      f"  | best old {best_old} / new {med[best_old] / med['new']:.2f}  new/copy {med['new'] / med['copy']:.2f}  | {verdict}"
                      f"  | checked {pick.numel()} rows; old:cumsum draws new's position in {same} of {rows * ndraw} draws{widened}", file=out)
                out.flush()
                v.clear()
                del x, cum, expo, quot, cdst, c64, ws
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--key", action="append", choices=list(DT), default=[])
    ap.add_argument("--warmup", type=int, default=2, help="calls of each variant before the timed ones")
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", action="append", default=[], metavar="ROWSxCOLSxNDRAW", help="these shapes instead of the five")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_bench: no GPU (no CPU fallback)")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shape] if a.shape else SHAPES
    out = open(a.out, "a") if a.out else sys.stdout
    main(a.reps, out, a.key or list(DT), shapes, a.warmup)
