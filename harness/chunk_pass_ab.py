#!/usr/bin/env python3
"""A/B of the chunked radix passes (csrc/chunk_pass.h: labsort_sort16_device's long rows and
labsort_sort64_device) against another build of liblabsort.so, usually the parent commit's
(output kept in profiles/chunk_pass.txt, part 2).

The shapes are those of §3.14 and §3.17:
  sort16  standard normals rounded to the type, descending: bf16 and f16 with positions at 1 x 2^28,
          2048 x 131072 and 5341 x 50257; bf16 keys only at the first two
  sort64  ascending: u64 over the full width, i64 in [0, 2^32) and f64 normals with positions at
          1 x 2^27 and 1024 x 131072, the first two at 32768 x 4096 (one workgroup per row); u64
          keys only at 1 x 2^27 and 32768 x 4096
Both builds are loaded in this process and called alternating, repetition by repetition, after two
warm-up calls each (device events around one call); ms, median [min, max].  `ok`: this build's
median minus the other's is no more than the other's max - min (the project's rule, §3.8).  Both
builds read and write the same buffers: with outputs of their own, two copies of one build differed
by up to 9 % on the eight-pass shapes, by where the outputs lay.  Both builds' outputs are compared
word for word, once per shape, and before any of it both builds' workspace sizes over a grid of
(rows, cols, positions) around every path and scan edge."""
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
from lds_classes_ab import entry, fmt, timed  # noqa: E402
from sort64_bench import KEY as KEY64, make as make64  # noqa: E402

DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}
# (entry, input, rows, cols, with positions)
SHAPES = ([("sort16", key, r, c, True) for key in ("bf16", "f16") for r, c in ((1, 1 << 28), (2048, 131072), (5341, 50257))]
          + [("sort16", "bf16", r, c, False) for r, c in ((1, 1 << 28), (2048, 131072))]
          + [("sort64", inp, r, c, True) for r, c in ((1, 1 << 27), (1024, 131072)) for inp in ("u64_full", "i64_lt2p32", "f64_normal")]
          + [("sort64", inp, 32768, 4096, True) for inp in ("u64_full", "i64_lt2p32")]
          + [("sort64", "u64_full", r, c, False) for r, c in ((1, 1 << 27), (32768, 4096))])


def workspace_sizes(builds, out):
    """Host-only: both builds' answers over rows x cols x positions; cols on both sides of each path
    edge, of whole chunks, and of 64 / 65 chunks (the serial and the workgroup scan)."""
    bad = total = 0
    for fam, edge in (("sort16", ls.segment_tile_keys()), ("sort64", ls.sort64_chunk_keys())):
        C = getattr(ls, fam + "_chunk_keys")()
        cols = sorted({1, edge - 1, edge, edge + 1, 2 * C, 2 * C + 1, 3 * C - 1, 3 * C, 64 * C - 1, 64 * C, 64 * C + 1, 65 * C, 65 * C + 1})
        f = {b: entry(lib, f"labsort_{fam}_workspace_bytes") for b, lib in builds.items()}
        for b in f:
            f[b].restype = ctypes.c_size_t
        for rows in (0, 1, 3, 67, 2048):
            for c in cols:
                for pos in (0, 1):
                    total += 1
                    got = {b: f[b](rows, c, pos) for b in f}
                    if got["this"] != got["other"]:
                        bad += 1
                        print(f"{fam} workspace_bytes({rows}, {c}, {pos}): other {got['other']}  this {got['this']}  DIFFER", file=out)
    print(f"# workspace sizes: {total} (rows, cols, positions) of both entries, {bad} differ", file=out)
    return bad


def main(reps, other, out, only):
    builds = {"other": ctypes.CDLL(other), "this": ls.lib}
    st = torch.cuda.current_stream().cuda_stream
    print(f"# chunked radix passes, 2 warm-up calls and {reps} alternating repetitions per build, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; this: {ls.version()}; other: {other}", file=out)
    if workspace_sizes(builds, out):
        sys.exit("chunk_pass_ab: the builds' workspace sizes differ")
    data = {}
    for fam, inp, rows, cols, pos in SHAPES:
        if only and fam not in only:
            continue
        n = rows * cols
        if (fam, inp) not in data:
            data.clear()
            if fam == "sort16":
                x = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
                x.normal_(generator=torch.Generator(device="cuda").manual_seed(0x5167EED))
                data[fam, inp] = x.to(DT16[inp])
                del x
            else:
                data[fam, inp] = make64(inp, 1 << 27)
        x = data[fam, inp][:n]
        kt = ls.KEY[inp if fam == "sort16" else KEY64[inp]]
        desc = 1 if fam == "sort16" else 0
        ws = torch.full((getattr(ls, fam + "_workspace_bytes")(rows, cols, pos),), 0xFF, dtype=torch.uint8, device="cuda")
        ko = torch.zeros_like(x)
        io = torch.zeros(n if pos else 1, dtype=torch.int32, device="cuda")
        f = {b: entry(lib, f"labsort_{fam}_device") for b, lib in builds.items()}
        call = {b: (lambda b=b: f[b](x.data_ptr(), rows, cols, desc, kt, ko.data_ptr(), io.data_ptr() if pos else None,
                                     ws.data_ptr(), ws.numel(), st)) for b in builds}
        got = {}
        for b, fn in call.items():
            ko.zero_()
            io.zero_()
            for _ in range(2):
                if fn() != 0:
                    sys.exit(f"chunk_pass_ab: {fam} {inp} {rows} x {cols}: the call returned an error")
            got[b] = (ko.view(torch.uint8).clone(), io.clone())
        same = all(torch.equal(u, v) for u, v in zip(got["this"], got["other"]))
        del got
        t = {b: [] for b in builds}
        for _ in range(reps):
            for b, fn in call.items():
                t[b].append(timed(fn))
        d = statistics.median(t["this"]) - statistics.median(t["other"])
        spread = max(t["other"]) - min(t["other"])
        print(f"{fam} {inp:<11}{rows:>6} x {cols:<10}{'positions' if pos else 'keys only':<10} other {fmt(t['other'])}  this {fmt(t['this'])}  "
              f"diff {d:+.4f}  other's spread {spread:.4f}  {'ok' if d <= spread else 'SLOWER'}  "
              f"outputs {'equal' if same else 'DIFFER'}", file=out)
        out.flush()
        del ko, io, ws


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the other build of liblabsort.so")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", nargs="*", default=[], help="only these entries (sort16 sort64)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chunk_pass_ab: no GPU (no CPU fallback)")
    main(a.reps, a.other, open(a.out, "a") if a.out else sys.stdout, a.only)
