#!/usr/bin/env python3
"""Segmented sort measurements on an MI355X (output kept as
profiles/segsort_bench.txt).

int32 keys (--key i32; uniform) or float32 keys (--key f32; standard normal), 2^28 in all, as
rows x cols for four row lengths, keys only and pairs:
  lds       labsort_sort_segments[_pairs]_device with max_segment_keys = cols (LDS path)
  general   the same call with max_segment_keys = 0 (two pair sorts of the whole array)
  copy      labsort_copy of the same keys: the 8 B/key floor
  torch     torch.sort(x.view(rows, cols), dim=1): an outside comparator, recorded only
  tile      labsort_tile_sort on the same buffer (cols = labsort_tile_keys() only): the same
            work when every segment is one aligned tile
Every variant of a shape is timed in turn, repetition by repetition (device events around
one call), after one warm-up each; median [min, max] ms over the repetitions.

--edges LIB[,LIB...]: the class-edge sweep.  Row lengths around the wave/block edges timed
with this build and with the given alternative builds of liblabsort.so (make
EXTRA=-DLABSORT_SEG_WAVE_KPT=.. / -DLABSORT_SEG_WAVE2_KPT=.. BUILD=build_x OUT=...: other
keys per lane, so other edges, of the two wave classes), alternating."""
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


def raw_call(lib, pairs):
    """The C entry of an alternative build, with the module's argument types."""
    f = lib.labsort_sort_segments_pairs_device if pairs else lib.labsort_sort_segments_device
    ref = ls.lib.labsort_sort_segments_pairs_device if pairs else ls.lib.labsort_sort_segments_device
    f.argtypes = ref.argtypes
    return f


def shapes_main(logn, reps, out, key="i32"):
    n = 1 << logn
    if key == "f32":
        keys = torch.empty(n, dtype=torch.float32, device="cuda")
        keys.normal_(generator=torch.Generator(device="cuda").manual_seed(0x5E65EED))
    else:
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        ls.fill(keys, n, seed=0x5E65EED, dist="u32")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    print(f"# segmented sort, {'float32' if key == 'f32' else 'int32'} keys, n = 2^{logn}, {reps} alternating repetitions, ms: median [min, max]", file=out)
    print(f"# device: {torch.cuda.get_device_name(0)}; {ls.version()}", file=out)
    for cols in (16, 256, 4096, 32768):
        rows = n // cols
        offs = ls.row_offsets(rows, cols)
        for pairs in (False, True):
            tile = ls.segment_pair_tile_keys() if pairs else ls.segment_tile_keys()
            ws_g = torch.zeros(ls.segments_workspace_bytes(n, rows, 0, pairs), dtype=torch.uint8, device="cuda")
            v = {}
            if cols <= tile:
                ws_l = torch.zeros(ls.segments_workspace_bytes(n, rows, cols, pairs), dtype=torch.uint8, device="cuda")
                if pairs:
                    v["lds"] = lambda: ls.sort_segments_pairs_device(keys, vals, ko, vo, n, offs, rows, cols, key=key, workspace=ws_l)
                else:
                    v["lds"] = lambda: ls.sort_segments_device(keys, ko, n, offs, rows, cols, key=key, workspace=ws_l)
            if pairs:
                v["general"] = lambda: ls.sort_segments_pairs_device(keys, vals, ko, vo, n, offs, rows, 0, key=key, workspace=ws_g)
            else:
                v["general"] = lambda: ls.sort_segments_device(keys, ko, n, offs, rows, 0, key=key, workspace=ws_g)
            v["copy"] = lambda: ls.copy(keys, ko, n)
            if not pairs:
                v["torch"] = lambda: torch.sort(keys.view(rows, cols), dim=1)
                if cols == ls.tile_keys() and key == "i32":
                    v["tile"] = lambda: ls.tile_sort(keys, ko, n, key="i32")
            else:
                v["torch"] = lambda: torch.sort(keys.view(rows, cols), dim=1, stable=True)
            t = alternate(v, reps)
            # the result of both paths, once, against torch
            exp = torch.sort(keys.view(rows, cols), dim=1, stable=True)
            for name in ("lds", "general"):
                if name in v:
                    ko.zero_()
                    v[name]()
                    ls.segments_workspace_status(ws_l if name == "lds" else ws_g)
                    assert torch.equal(ko.view(rows, cols), exp.values), (cols, pairs, name)
                    if pairs:
                        assert torch.equal(vo.view(rows, cols).long(), exp.indices + offs[:-1].long().unsqueeze(1)), (cols, pairs, name)
            print(f"{rows:>9} x {cols:<6} {'pairs' if pairs else 'keys '}  " +
                  "  ".join(f"{k} {fmt(ts)}" for k, ts in t.items()), file=out)
            out.flush()
            del ws_g, exp


def edges_main(logn, reps, libs, out):
    n = 1 << logn
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    ls.fill(keys, n, seed=0x5E65EED, dist="u32")
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    builds = {"this": ls.lib}
    for path in libs:
        builds[os.path.basename(path)] = ctypes.CDLL(path)
    st = torch.cuda.current_stream().cuda_stream
    print(f"# class-edge sweep, int32 keys, n = 2^{logn}, {reps} alternating repetitions, ms: median [min, max]", file=out)
    for name, lib in builds.items():
        e = (ctypes.c_size_t * 8)()
        k = lib.labsort_segment_class_edges(0, e, 8)
        print(f"# build {name}: class edges {[int(e[i]) for i in range(k)]}", file=out)
    for cols in (64, 128, 192, 256, 384, 512, 768, 1024, 2048):
        rows = n // cols
        nn = rows * cols
        offs = ls.row_offsets(rows, cols)
        for pairs in (False, True):
            ws = torch.zeros(ls.segments_workspace_bytes(nn, rows, cols, pairs), dtype=torch.uint8, device="cuda")
            v = {}
            for name, lib in builds.items():
                f = raw_call(lib, pairs)
                if pairs:
                    v[name] = (lambda f=f: f(keys.data_ptr(), vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), nn,
                                             offs.data_ptr(), rows, cols, 1, ws.data_ptr(), ws.numel(), st))
                else:
                    v[name] = (lambda f=f: f(keys.data_ptr(), ko.data_ptr(), nn, offs.data_ptr(), rows, cols, 1,
                                             ws.data_ptr(), ws.numel(), st))
            t = alternate(v, reps)
            print(f"{rows:>9} x {cols:<6} {'pairs' if pairs else 'keys '}  " +
                  "  ".join(f"{k} {fmt(ts)}" for k, ts in t.items()), file=out)
            out.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--key", choices=["i32", "f32"], default="i32", help="f32: standard-normal float32 keys")
    ap.add_argument("--edges", default="", help="comma-separated alternative builds of liblabsort.so")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("segsort_bench: no GPU (no CPU fallback)")
    out = open(a.out, "a") if a.out else sys.stdout
    if a.edges:
        edges_main(a.logn, a.reps, [p for p in a.edges.split(",") if p], out)
    else:
        shapes_main(a.logn, a.reps, out, a.key)
